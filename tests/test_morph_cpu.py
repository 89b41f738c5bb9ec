"""vr_morph's host side, the checks that need no GPU: the conditions the shared
input must meet (half widths, an in-place sweep and a zero-padded erode all
give other bytes); vr_brush_morph_apply against the numpy restatement of the
erode / dilate brush (tests/morph_spec.py) on every brush of paint_spec.BRUSHES
x op x half width x falloff; edge volumes; a constant channel; the order
erode <= old <= dilate; refusals; prototypes and exports."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brush(centre, radius, falloff=0, strength=ms.STRENGTH, op=0):
    import volumetricrenderer_amd as vr
    return vr.make_brush(centre, radius, op, falloff, (1, 2, 3, 4), strength)


@pytest.fixture(scope="module")
def base():
    return ms.morph_volume()


def test_the_input_tells_wrong_implementations_apart(base):
    """Asserted before anything is compared with the library: on this volume another half width, an in-place
    sweep and (for erode) zero padding instead of clamping each give other bytes."""
    assert base.shape == (ps.NZ, ps.NY, ps.NX, 4) and base.min() == 0 and base.max() <= 254
    ch = base[..., 0]
    for op, _ in ms.OPS:
        e = {h: ms.cube_extrema(ch, h, op) for h in ms.HALF_WIDTHS}
        assert (e[1] != e[2]).mean() > 0.5 and (e[2] != e[3]).mean() > 0.5, "the half widths are too close"
        swept = ms.gauss_seidel_morph(base, op, 1)
        want = np.stack([ms.cube_extrema(base[..., c], 1, op) for c in range(4)], axis=-1)
        assert (swept != want).mean() > 0.5, "the in-place sweep is too close to the specification"
    zero = ms.cube_extrema(ch, 1, ms.ERODE, pad_mode="constant")
    clamp = ms.cube_extrema(ch, 1, ms.ERODE)
    faces = np.ones(ch.shape, bool)
    faces[1:-1, 1:-1, 1:-1] = False
    assert (zero != clamp)[faces].any() and not (zero != clamp)[~faces].any(), "zero padding shows on the faces only"
    assert (zero != clamp).mean() > 0.1


@pytest.mark.parametrize("falloff,fname", ps.FALLOFFS, ids=[n for _, n in ps.FALLOFFS])
@pytest.mark.parametrize("h", ms.HALF_WIDTHS)
@pytest.mark.parametrize("op,oname", ms.OPS, ids=[n for _, n in ms.OPS])
@pytest.mark.parametrize("name", list(ps.BRUSHES))
def test_morph_apply_matches_the_numpy_restatement(base, name, op, oname, h, falloff, fname):
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES[name]
    want = ms.spec_morph(base, centre, radius, op, h, falloff)
    got = vr.brush_morph_apply(brush(centre, radius, falloff), op, h, base.copy())
    assert_exact(got, want)
    # the conditions on the inputs: a weaker input must not hide a failure
    inside, _ = ps.spec_weights(base.shape[:3], centre, radius, falloff)
    assert (want[..., 3] == base[..., 3]).all(), "channel A has strength 0"
    assert (want[~inside] == base[~inside]).all()
    if name == "miss":
        assert not inside.any() and (want == base).all()
        return
    assert (want != base).any(), "no byte changed where the brush hits"
    if name in ("corner", "far_corner"):
        assert (ms.clamped_axes(base.shape[:3], centre, radius, h) == 3).any(), "no cube clamped on three axes"


def test_a_whole_volume_morph_is_the_cube_extremum(base):
    """`whole`, hard edge, full strength: every byte becomes its cube's extremum (the Jacobi result), and
    erode <= old <= dilate holds per byte."""
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES["whole"]
    inside, _ = ps.spec_weights(base.shape[:3], centre, radius, 0)
    assert inside.all()
    for h in ms.HALF_WIDTHS:
        got = {}
        for op, _ in ms.OPS:
            want = np.stack([ms.cube_extrema(base[..., c], h, op) for c in range(4)], axis=-1).astype(np.uint8)
            got[op] = vr.brush_morph_apply(brush(centre, radius, 0, ms.FULL), op, h, base.copy())
            assert_exact(got[op], want)
        assert (got[ms.ERODE] <= base).all() and (base <= got[ms.DILATE]).all()
        assert (got[ms.ERODE] < base).any() and (base < got[ms.DILATE]).any()


def test_edge_volumes():
    import volumetricrenderer_amd as vr
    one = np.array([[[[9, 200, 0, 255]]]], np.uint8)
    rng = np.random.default_rng(11)
    thin = rng.integers(0, 256, size=(1, 3, 2, 4), dtype=np.uint8)   # 2 x 3 x 1: thinner than any halo
    vol = rng.integers(0, 256, size=(9, 7, 12, 4), dtype=np.uint8)
    vol[..., 1] = 77                                                 # a constant channel stays constant
    for op, _ in ms.OPS:
        for h in ms.HALF_WIDTHS:
            for falloff in (0, 1):
                got = vr.brush_morph_apply(brush((0, 0, 0), (255, 255, 255), falloff, ms.FULL), op, h, one.copy())
                assert_exact(got, one)   # every neighbour is the texel itself
                assert_exact(ms.spec_morph(one, (0, 0, 0), (255, 255, 255), op, h, falloff, ms.FULL), one)
            want = ms.spec_morph(thin, (1, 1, 0), (4, 4, 4), op, h, 1, ms.FULL)
            assert (want != thin).any()
            assert_exact(vr.brush_morph_apply(brush((1, 1, 0), (4, 4, 4), 1, ms.FULL), op, h, thin.copy()), want)
            got = vr.brush_morph_apply(brush((5, 3, 4), (6, 6, 6), 1, ms.FULL), op, h, vol.copy())
            assert (got[..., 1] == 77).all()
            assert (got[..., 0] != vol[..., 0]).any()
            assert_exact(got, ms.spec_morph(vol, (5, 3, 4), (6, 6, 6), op, h, 1, ms.FULL))
    with pytest.raises(ValueError):
        vr.brush_morph_apply(brush((0, 0, 0), (1, 1, 1)), 0, 1, np.zeros((2, 2, 2, 3), np.uint8))


def test_refusals_leave_the_array_untouched():
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    vol = np.random.default_rng(5).integers(0, 256, size=(4, 4, 4, 4), dtype=np.uint8)
    keep = vol.copy()
    vp = vol.ctypes.data_as(ctypes.c_void_p)
    good = brush((1, 1, 1), (2, 2, 2))
    for op in (0, 1):
        assert lib.vr_brush_morph_apply(ctypes.byref(good), op, 1, vp, 4, 4, 4) == 0
        assert (vol != keep).any()
        vol[...] = keep
    bad = [(brush((1, 1, 1), (2, 2, 2), op=1), 0, 1), (brush((1, 1, 1), (2, 2, 2), op=2), 1, 1),
           (brush((1, 1, 1), (2, 2, 2), op=3), 0, 1),
           (good, 2, 1), (good, -1, 1), (good, 2**31 - 1, 1), (good, -2**31, 1),
           (good, 0, 0), (good, 1, 4), (good, 0, -1), (good, 1, 2**31 - 1), (good, 0, -2**31),
           (brush((1, 1, 1), (2, -1, 2)), 0, 1), (brush((1, 1, 1), (256, 2, 2)), 1, 1),
           (brush((1, 1, 1), (2, 2, 2), falloff=2), 0, 1)]
    for k in range(2):
        b = brush((1, 1, 1), (2, 2, 2))
        b.reserved[k] = 1
        bad.append((b, k, 1))
    for b, op, h in bad:
        assert lib.vr_brush_morph_apply(ctypes.byref(b), op, h, vp, 4, 4, 4) == 1, (b.op, op, h)   # VR_ERR_INVALID
        assert "vr_brush_morph_apply:" in lib.vr_last_error().decode()
        assert lib.vr_morph(None, ctypes.byref(b), op, h, None) == 1
        assert (vol == keep).all()
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert lib.vr_brush_morph_apply(ctypes.byref(good), 0, 1, vp, *dims) == 1
    for name, args in (("vr_brush_morph_apply", (None, 0, 1, vp, 4, 4, 4)),
                       ("vr_brush_morph_apply", (ctypes.byref(good), 0, 1, None, 4, 4, 4)),
                       ("vr_morph", (None, ctypes.byref(good), 0, 1, None)),
                       ("vr_morph", (ctypes.c_void_p(8), None, 0, 1, None))):
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
    for name, nargs in (("vr_morph", 5), ("vr_brush_morph_apply", 7)):
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
        m = re.search(r"vr_status\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib._SIGS[name][1]), name
        assert _lib._SIGS[name][0] is ctypes.c_int
    assert re.search(r"#define\s+VR_MORPH_MAX_HALF\s+3\b", src) and vr.MORPH_MAX_HALF == 3
    assert re.search(r"VR_MORPH_ERODE\s*=\s*0\s*,\s*VR_MORPH_DILATE\s*=\s*1", src)
    assert (vr.MORPH_ERODE, vr.MORPH_DILATE) == (0, 1)
    assert lib.vr_abi_version() == 2
    assert callable(vr.Renderer.morph) and callable(vr.brush_morph_apply)
    for name in ("brush_morph_apply", "MORPH_ERODE", "MORPH_DILATE", "MORPH_MAX_HALF"):
        assert name in vr.__all__
    hpp = open(os.path.join(ROOT, "include", "vr_renderer.hpp")).read()
    assert "vr_morph(" in hpp and "vr_brush_morph_apply(" in hpp
