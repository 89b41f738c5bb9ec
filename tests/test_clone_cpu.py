"""vr_clone's and vr_stamp's host side, the checks that need no GPU: the
conditions the shared inputs must meet; vr_brush_clone_apply against the numpy
restatement (tests/clone_spec.py) on every brush of paint_spec.BRUSHES x map x
op x falloff; vr_brush_stamp_apply and vr_stamp_box against it on the stamp
cases; the identity; the mirror applied twice; refusals; prototypes and
exports."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clone_spec as cs  # noqa: E402
import paint_spec as ps  # noqa: E402
from brush_harness import assert_exact, base  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (ps.NX, ps.NY, ps.NZ)


def brush(centre, radius, op=ps.SET, falloff=0, strength=cs.STRENGTH):
    import volumetricrenderer_amd as vr
    return vr.make_brush(centre, radius, op, falloff, (1, 2, 3, 4), strength)


def test_the_inputs_tell_wrong_implementations_apart(base):
    """Asserted before anything is compared with the library: with `interior`, the maps named direct are the ones
    whose source misses the box; for each axis an ascending or a descending in-place sweep gets a push wrong;
    `huge` and `edge` read a corner, which a 32-bit sum would not; the offsets of `touch` and `overlap1` differ
    by the one column that decides the path."""
    centre, radius = ps.BRUSHES["interior"]
    for name, f in cs.MAPS.items():
        offset, mirror = f(centre)
        assert cs.spec_direct(centre, radius, offset, mirror) == (name in cs.DIRECT_MAPS), name
    for name in cs.PUSHES:
        offset, _ = cs.MAPS[name](centre)
        want = cs.spec_clone(base, centre, radius, offset, (0, 0, 0), ps.SET, 0, cs.FULL)
        wrong = [(cs.sweep_clone(base, centre, radius, offset, asc) != want).any() for asc in (True, False)]
        assert sorted(wrong) == [False, True], (name, wrong)
    sx = cs.source_index(ps.NX, cs.INT32_MAX, 0)
    sy = cs.source_index(ps.NY, cs.INT32_MIN, 0)
    assert (sx == ps.NX - 1).all() and (sy == 0).all()
    wrapped = (np.arange(ps.NX, dtype=np.int64) + cs.INT32_MAX + 2**31) % 2**32 - 2**31   # what int32 would give
    assert (np.clip(wrapped, 0, ps.NX - 1) != sx).any()
    assert (cs.source_index(ps.NX, -30, 0)[:21] == 0).all() and (cs.source_index(ps.NZ, -60, 0) == 0).all()


@pytest.mark.parametrize("mname", list(cs.MAPS))
@pytest.mark.parametrize("name", list(ps.BRUSHES))
def test_clone_apply_matches_the_numpy_restatement(base, name, mname):
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES[name]
    offset, mirror = cs.MAPS[mname](centre)
    inside, _ = ps.spec_weights(base.shape[:3], centre, radius, 0)
    sx, sy, sz = (cs.source_index(n, o, m) for n, o, m in zip(DIMS, offset, mirror))
    own = [s == np.arange(n) for s, n in zip((sx, sy, sz), DIMS)]
    own_source = (own[0][None, None, :] & own[1][None, :, None] & own[2][:, None, None])[inside]
    for op, _ in ps.OPS:
        for falloff, _ in ps.FALLOFFS:
            want = cs.spec_clone(base, centre, radius, offset, mirror, op, falloff)
            got = vr.brush_clone_apply(brush(centre, radius, op, falloff), vr.make_clone_map(offset, mirror), base.copy())
            assert_exact(got, want)
            # the conditions on the inputs: a weaker input must not hide a failure
            assert (want[..., 3] == base[..., 3]).all(), "channel A has strength 0"
            assert (want[~inside] == base[~inside]).all()
            if name == "miss":
                assert not inside.any() and (want == base).all()
            elif own_source.all():   # the identity, or the centre texel under a mirror about itself
                assert mname in ("identity", "mirror_x", "mirror_xyz")
                assert (want == base).all() == (op == ps.SET)
            elif falloff == 0:       # (on a smooth rim the weight may be 1, which rounds to the old byte)
                assert (want != base).any(), "no byte changed where the brush hits"


def test_the_identity_set_leaves_the_array_unchanged(base):
    import volumetricrenderer_amd as vr
    for name, (centre, radius) in ps.BRUSHES.items():
        for falloff in (0, 1):
            for strength in (cs.STRENGTH, cs.FULL, (7, 0, 200, 255)):
                got = vr.brush_clone_apply(brush(centre, radius, ps.SET, falloff, strength), vr.make_clone_map(), base.copy())
                assert_exact(got, base)


def test_a_mirror_twice_restores_and_once_is_symmetric(base):
    """Hard edge, strength 255, `interior`, mirror_x: the box becomes x-symmetric inside the ellipsoid (which is
    symmetric about its own centre plane), and a second application restores every byte."""
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES["interior"]
    offset, mirror = cs.MAPS["mirror_x"](centre)
    b, m = brush(centre, radius, ps.SET, 0, cs.FULL), vr.make_clone_map(offset, mirror)
    once = vr.brush_clone_apply(b, m, base.copy())
    assert_exact(once, cs.spec_clone(base, centre, radius, offset, mirror, ps.SET, 0, cs.FULL))
    assert (once != base).any()
    inside, _ = ps.spec_weights(base.shape[:3], centre, radius, 0)
    (ox, oy, oz), (ex, ey, ez) = ps.spec_box(centre, radius)
    box, was = once[oz:oz + ez, oy:oy + ey, ox:ox + ex], base[oz:oz + ez, oy:oy + ey, ox:ox + ex]
    ins = inside[oz:oz + ez, oy:oy + ey, ox:ox + ex]
    assert (ins == ins[:, :, ::-1]).all()
    assert (box[ins] == was[:, :, ::-1][ins]).all(), "the box is not the mirror image of what it was"
    assert_exact(vr.brush_clone_apply(b, m, once.copy()), base)


@pytest.mark.parametrize("sname", list(cs.STAMPS))
def test_stamp_apply_and_stamp_box_match_the_numpy_restatement(base, sname):
    import volumetricrenderer_amd as vr
    bname, extent, origin = cs.STAMPS[sname]
    centre, radius = ps.BRUSHES[bname]
    stamp = cs.stamp_bytes(extent)
    want_box = cs.spec_stamp_box(centre, radius, origin, extent)
    assert vr.stamp_box(brush(centre, radius), (origin, extent), DIMS) == want_box
    assert (want_box is None) == (sname in ("miss", "outside"))
    if sname == "covers":
        assert want_box == ps.spec_box(centre, radius)
    if sname in ("two_faces", "far_faces"):
        assert want_box != ps.spec_box(centre, radius) and want_box[1] != tuple(extent)
    if sname == "smaller":
        assert want_box == (tuple(origin), tuple(extent)) != ps.spec_box(centre, radius)
    for op, _ in ps.OPS:
        for falloff, _ in ps.FALLOFFS:
            want = cs.spec_stamp(base, stamp, origin, centre, radius, op, falloff)
            got = vr.brush_stamp_apply(brush(centre, radius, op, falloff), stamp, origin, base.copy())
            assert_exact(got, want)
            assert (want[..., 3] == base[..., 3]).all()
            assert (want != base).any() == (want_box is not None)
            if want_box is not None:
                (ox, oy, oz), (ex, ey, ez) = want_box
                outside = np.ones(base.shape[:3], bool)
                outside[oz:oz + ez, oy:oy + ey, ox:ox + ex] = False
                assert (want[outside] == base[outside]).all(), "a byte outside vr_stamp_box changed"


def test_a_stamp_of_the_volumes_own_box_is_a_clone(base):
    """A box cut out of the volume and stamped at an offset is the clone with that offset, where the box covers
    the brush: the two definitions agree."""
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES["interior"]
    (ox, oy, oz), (ex, ey, ez) = ps.spec_box(centre, radius)
    cut = np.ascontiguousarray(base[oz:oz + ez, oy:oy + ey, ox + 12:ox + 12 + ex])
    for op, _ in ps.OPS:
        got = vr.brush_stamp_apply(brush(centre, radius, op, 1), cut, (ox, oy, oz), base.copy())
        assert_exact(got, cs.spec_clone(base, centre, radius, (12, 0, 0), (0, 0, 0), op, 1))


def test_refusals_leave_the_array_untouched():
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    vol = np.random.default_rng(5).integers(0, 256, size=(4, 4, 4, 4), dtype=np.uint8)
    keep = vol.copy()
    vp = vol.ctypes.data_as(ctypes.c_void_p)
    stamp = np.random.default_rng(6).integers(0, 256, size=(2, 2, 2, 4), dtype=np.uint8)
    sp = stamp.ctypes.data_as(ctypes.c_void_p)
    good, gmap, gbox = brush((1, 1, 1), (2, 2, 2)), vr.make_clone_map((1, 0, 0)), _lib.Box(0, 0, 0, 2, 2, 2)
    o, e = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    assert lib.vr_brush_clone_apply(ctypes.byref(good), ctypes.byref(gmap), vp, 4, 4, 4) == 0
    assert (vol != keep).any()
    vol[...] = keep
    assert lib.vr_brush_stamp_apply(ctypes.byref(good), sp, ctypes.byref(gbox), vp, 4, 4, 4) == 0
    assert (vol != keep).any()
    vol[...] = keep
    bad_brushes = [brush((1, 1, 1), (2, 2, 2), op=3), brush((1, 1, 1), (2, 2, 2), op=-1),
                   brush((1, 1, 1), (2, -1, 2)), brush((1, 1, 1), (256, 2, 2)), brush((1, 1, 1), (2, 2, 2), falloff=2)]
    for k in range(2):
        b = brush((1, 1, 1), (2, 2, 2))
        b.reserved[k] = 1
        bad_brushes.append(b)
    bad_maps = [vr.make_clone_map((0, 0, 0), (2, 0, 0)), vr.make_clone_map((0, 0, 0), (0, -1, 0)),
                vr.make_clone_map((0, 0, 0), (0, 0, 2**31 - 1))]
    for k in range(2):
        m = vr.make_clone_map((1, 0, 0))
        m.reserved[k] = 5
        bad_maps.append(m)
    bad_boxes = [_lib.Box(0, 0, 0, 0, 2, 2), _lib.Box(0, 0, 0, 2, -1, 2), _lib.Box(0, 0, 0, 2, 2, -2**31)]
    for b, m in [(b, gmap) for b in bad_brushes] + [(good, m) for m in bad_maps]:
        assert lib.vr_brush_clone_apply(ctypes.byref(b), ctypes.byref(m), vp, 4, 4, 4) == 1   # VR_ERR_INVALID
        assert "vr_brush_clone_apply:" in lib.vr_last_error().decode()
        assert lib.vr_clone(None, ctypes.byref(b), ctypes.byref(m), None) == 1
        assert (vol == keep).all()
    for b, box in [(b, gbox) for b in bad_brushes] + [(good, box) for box in bad_boxes]:
        assert lib.vr_brush_stamp_apply(ctypes.byref(b), sp, ctypes.byref(box), vp, 4, 4, 4) == 1
        assert "vr_brush_stamp_apply:" in lib.vr_last_error().decode()
        assert lib.vr_stamp_box(ctypes.byref(b), ctypes.byref(box), 4, 4, 4, o, e) == 1
        assert "vr_stamp_box:" in lib.vr_last_error().decode()
        assert lib.vr_stamp(None, ctypes.byref(b), ctypes.c_void_p(8), ctypes.byref(box), None) == 1
        assert (vol == keep).all()
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert lib.vr_brush_clone_apply(ctypes.byref(good), ctypes.byref(gmap), vp, *dims) == 1
        assert lib.vr_brush_stamp_apply(ctypes.byref(good), sp, ctypes.byref(gbox), vp, *dims) == 1
        assert lib.vr_stamp_box(ctypes.byref(good), ctypes.byref(gbox), *dims, o, e) == 1
    gb, gm, gx = ctypes.byref(good), ctypes.byref(gmap), ctypes.byref(gbox)
    for name, args in (("vr_brush_clone_apply", (None, gm, vp, 4, 4, 4)), ("vr_brush_clone_apply", (gb, None, vp, 4, 4, 4)),
                       ("vr_brush_clone_apply", (gb, gm, None, 4, 4, 4)),
                       ("vr_brush_stamp_apply", (None, sp, gx, vp, 4, 4, 4)), ("vr_brush_stamp_apply", (gb, None, gx, vp, 4, 4, 4)),
                       ("vr_brush_stamp_apply", (gb, sp, None, vp, 4, 4, 4)), ("vr_brush_stamp_apply", (gb, sp, gx, None, 4, 4, 4)),
                       ("vr_stamp_box", (None, gx, 4, 4, 4, o, e)), ("vr_stamp_box", (gb, None, 4, 4, 4, o, e)),
                       ("vr_stamp_box", (gb, gx, 4, 4, 4, None, e)), ("vr_stamp_box", (gb, gx, 4, 4, 4, o, None)),
                       ("vr_clone", (None, gb, gm, None)), ("vr_clone", (ctypes.c_void_p(8), None, gm, None)),
                       ("vr_clone", (ctypes.c_void_p(8), gb, None, None)),
                       ("vr_stamp", (None, gb, ctypes.c_void_p(8), gx, None)),
                       ("vr_stamp", (ctypes.c_void_p(8), None, ctypes.c_void_p(8), gx, None)),
                       ("vr_stamp", (ctypes.c_void_p(8), gb, None, gx, None)),
                       ("vr_stamp", (ctypes.c_void_p(8), gb, ctypes.c_void_p(8), None, None))):
        assert getattr(lib, name)(*args) == 1, name
        msg = lib.vr_last_error().decode()
        assert name + ":" in msg and "null" in msg, msg
    assert (vol == keep).all()
    with pytest.raises(ValueError):
        vr.brush_clone_apply(good, gmap, np.zeros((2, 2, 2, 3), np.uint8))
    with pytest.raises(ValueError):
        vr.brush_stamp_apply(good, np.zeros((0, 2, 2, 4), np.uint8), (0, 0, 0), vol)


def test_prototypes_exports_and_signatures():
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vr_[a-z_0-9]+)\s*\(", src))
    for name, nargs in (("vr_clone", 4), ("vr_brush_clone_apply", 6), ("vr_stamp", 5), ("vr_brush_stamp_apply", 7),
                        ("vr_stamp_box", 7)):
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
        m = re.search(r"vr_status\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib._SIGS[name][1]), name
        assert _lib._SIGS[name][0] is ctypes.c_int
    assert ctypes.sizeof(_lib.CloneMap) == 32 and re.search(r"\}\s*vr_clone_map\s*;", src)
    assert lib.vr_abi_version() == 2
    for name in ("clone", "stamp"):
        assert callable(getattr(vr.Renderer, name))
    for name in ("brush_clone_apply", "brush_stamp_apply", "stamp_box", "make_clone_map", "CloneMap"):
        assert name in vr.__all__ and hasattr(vr, name)
    hpp = open(os.path.join(ROOT, "include", "vr_renderer.hpp")).read()
    for call in ("vr_clone(", "vr_stamp(", "vr_brush_clone_apply(", "vr_brush_stamp_apply(", "vr_stamp_box("):
        assert call in hpp


def test_header_and_struct_compile_as_c(tmp_path):
    """include/vr.h with the new declarations is C99, and vr_clone_map is 32 bytes there too."""
    import subprocess
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "vr.h"\nint main(void){printf("%zu\\n", sizeof(vr_clone_map));return 0;}\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["32"]
