"""vr_blur's host side, the checks that need no GPU: vr_brush_blur_apply against
the numpy restatement of the box-filter brush (tests/blur_spec.py) on every
brush of paint_spec.BRUSHES x half width x falloff; the conditions those inputs
must meet (clamped neighbourhoods, a byte changed, a Gauss-Seidel sweep that
differs); edge volumes; refusals; prototypes and exports."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blur_spec as bs  # noqa: E402
import paint_spec as ps  # noqa: E402
from brush_harness import assert_exact, base  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vr_blur", "vr_brush_blur_apply")


def brush(centre, radius, falloff=0, strength=bs.STRENGTH, op=0):
    import volumetricrenderer_amd as vr
    return vr.make_brush(centre, radius, op, falloff, (1, 2, 3, 4), strength)


@pytest.mark.parametrize("falloff,fname", ps.FALLOFFS, ids=[n for _, n in ps.FALLOFFS])
@pytest.mark.parametrize("h", bs.HALF_WIDTHS)
@pytest.mark.parametrize("name", list(ps.BRUSHES))
def test_blur_apply_matches_the_numpy_restatement(base, name, h, falloff, fname):
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES[name]
    want = bs.spec_blur(base, centre, radius, h, falloff)
    got = vr.brush_blur_apply(brush(centre, radius, falloff), h, base.copy())
    assert_exact(got, want)
    # the conditions on the inputs: a weaker input must not hide a failure
    inside, _ = ps.spec_weights(base.shape[:3], centre, radius, falloff)
    assert (want[..., 3] == base[..., 3]).all(), "channel A has strength 0"
    assert (want[~inside] == base[~inside]).all()
    if name == "miss":
        assert not inside.any() and (want == base).all()
        return
    assert (want != base).any()
    if name in ("corner", "far_corner"):
        assert (bs.clamped_axes(base.shape[:3], centre, radius, h) == 3).any(), "no neighbourhood clamped on three axes"
    if name in ("interior", "texel"):
        # the neighbourhood leaves the brush's box (radius < h on some axis, or always for `texel`) but not the volume
        assert (bs.clamped_axes(base.shape[:3], centre, radius, h)[inside] == 0).all()


def test_an_in_place_sweep_differs_from_the_specification(base):
    """`whole`, hard edge, full strength, h = 1: every texel becomes its mean.  A sequential in-place sweep
    (Gauss-Seidel) gives other bytes than the Jacobi specification, so an implementation that is one cannot pass."""
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES["whole"]
    full = (255, 255, 255, 255)
    inside, _ = ps.spec_weights(base.shape[:3], centre, radius, 0)
    assert inside.all()
    want = bs.spec_blur(base, centre, radius, 1, 0, full)
    assert_exact(want, np.stack([bs.box_means(base[..., c], 1) for c in range(4)], axis=-1).astype(np.uint8))
    swept = bs.gauss_seidel_blur(base, 1)
    assert (swept != want).mean() > 0.5, "the in-place sweep is too close to the specification to tell them apart"
    assert_exact(vr.brush_blur_apply(brush(centre, radius, 0, full), 1, base.copy()), want)


def test_edge_volumes():
    import volumetricrenderer_amd as vr
    one = np.array([[[[9, 200, 0, 255]]]], np.uint8)
    for h in bs.HALF_WIDTHS:
        for falloff in (0, 1):
            got = vr.brush_blur_apply(brush((0, 0, 0), (255, 255, 255), falloff, (255,) * 4), h, one.copy())
            assert_exact(got, one)   # every neighbour is the texel itself
            assert_exact(bs.spec_blur(one, (0, 0, 0), (255, 255, 255), h, falloff, (255,) * 4), one)
    rng = np.random.default_rng(11)
    thin = rng.integers(0, 256, size=(1, 3, 2, 4), dtype=np.uint8)   # 2 x 3 x 1: thinner than any halo
    for h in bs.HALF_WIDTHS:
        want = bs.spec_blur(thin, (1, 1, 0), (4, 4, 4), h, 1, (255, 255, 255, 255))
        assert (want != thin).any()
        assert_exact(vr.brush_blur_apply(brush((1, 1, 0), (4, 4, 4), 1, (255,) * 4), h, thin.copy()), want)
    vol = rng.integers(0, 256, size=(9, 7, 12, 4), dtype=np.uint8)
    vol[..., 1] = 77                                                 # a constant channel stays constant
    for h in bs.HALF_WIDTHS:
        got = vr.brush_blur_apply(brush((5, 3, 4), (6, 6, 6), 1, (255,) * 4), h, vol.copy())
        assert (got[..., 1] == 77).all()
        assert (got[..., 0] != vol[..., 0]).any()
        assert_exact(got, bs.spec_blur(vol, (5, 3, 4), (6, 6, 6), h, 1, (255,) * 4))
    with pytest.raises(ValueError):
        vr.brush_blur_apply(brush((0, 0, 0), (1, 1, 1)), 1, np.zeros((2, 2, 2, 3), np.uint8))


def test_refusals_leave_the_array_untouched():
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    vol = np.random.default_rng(5).integers(0, 256, size=(4, 4, 4, 4), dtype=np.uint8)
    keep = vol.copy()
    vp = vol.ctypes.data_as(ctypes.c_void_p)
    good = brush((1, 1, 1), (2, 2, 2))
    assert lib.vr_brush_blur_apply(ctypes.byref(good), 1, vp, 4, 4, 4) == 0
    assert (vol != keep).any()
    vol[...] = keep
    bad = [(brush((1, 1, 1), (2, 2, 2), op=1), 1), (brush((1, 1, 1), (2, 2, 2), op=2), 1), (brush((1, 1, 1), (2, 2, 2), op=3), 1),
           (good, 0), (good, 4), (good, -1), (good, 2**31 - 1),
           (brush((1, 1, 1), (2, -1, 2)), 1), (brush((1, 1, 1), (256, 2, 2)), 1), (brush((1, 1, 1), (2, 2, 2), falloff=2), 1)]
    for k in range(2):
        b = brush((1, 1, 1), (2, 2, 2))
        b.reserved[k] = 1
        bad.append((b, 1))
    for b, h in bad:
        assert lib.vr_brush_blur_apply(ctypes.byref(b), h, vp, 4, 4, 4) == 1, (b.op, h)   # VR_ERR_INVALID
        assert "vr_brush_blur_apply:" in lib.vr_last_error().decode()
        assert lib.vr_blur(None, ctypes.byref(b), h, None) == 1
        assert (vol == keep).all()
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert lib.vr_brush_blur_apply(ctypes.byref(good), 1, vp, *dims) == 1
    for name, args in (("vr_brush_blur_apply", (None, 1, vp, 4, 4, 4)), ("vr_brush_blur_apply", (ctypes.byref(good), 1, None, 4, 4, 4)),
                       ("vr_blur", (None, ctypes.byref(good), 1, None)), ("vr_blur", (ctypes.c_void_p(8), None, 1, None))):
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
    for name, nargs in (("vr_blur", 4), ("vr_brush_blur_apply", 6)):
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
        m = re.search(r"vr_status\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib._SIGS[name][1]), name
        assert _lib._SIGS[name][0] is ctypes.c_int
    assert re.search(r"#define\s+VR_BLUR_MAX_HALF\s+3\b", src) and vr.BLUR_MAX_HALF == 3
    assert lib.vr_abi_version() == 2
    assert callable(vr.Renderer.blur) and callable(vr.brush_blur_apply)
    hpp = open(os.path.join(ROOT, "include", "vr_renderer.hpp")).read()
    assert "vr_blur(" in hpp and "vr_brush_blur_apply(" in hpp
