"""vr_paint_stroke's host companions, the checks that need no GPU: vr_brush_line
against a numpy int64 restatement, vr_boxes_coalesce against a Python
restatement of its rule (volumes in place of vr_rects_coalesce's areas), the
vr_box layout in the header and its ctypes mirror, the prototypes and exports,
and the argument checks of vr_paint_stroke that come before any device work.
The reference for a stroke itself is brush_apply in a loop (tests/paint_spec.py
is the reference for brush_apply): the GPU tests compare against it."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paint_spec as ps  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vr_paint_stroke", "vr_brush_line", "vr_boxes_coalesce")


def brush(centre, radius=(3, 2, 4), op=1, falloff=1, value=ps.VALUE, strength=ps.STRENGTH):
    import volumetricrenderer_amd as vr
    return vr.make_brush(centre, radius, op, falloff, value, strength)


# ---- vr_brush_line ---------------------------------------------------------------------------
def spec_line(centre, to, spacing, skip_first=False):
    """include/vr.h in numpy int64: the centres of the dabs."""
    c, t = np.array(centre, np.int64), np.array(to, np.int64)
    d = t - c
    n = max(1, int(-(-np.abs(d).max() // spacing)))
    i = np.arange(1 if skip_first else 0, n + 1, dtype=np.int64)[:, None]
    return c + np.floor_divide(2 * i * d + n, 2 * n)   # numpy's // is floor division


def centres(dabs):
    return np.array([list(b.centre) for b in dabs], np.int64).reshape(len(dabs), 3)


@pytest.mark.parametrize("signs", list(itertools.product((1, -1), repeat=3)), ids=lambda s: "".join("+-"[v < 0] for v in s))
def test_brush_line_all_direction_signs(signs):
    import volumetricrenderer_amd as vr
    b = brush((10, -4, 7))
    for lengths, spacing in (((23, 9, 14), 4), ((5, 31, 30), 7), ((1, 2, 3), 1), ((100, 99, 1), 3)):
        to = tuple(c + s * l for c, s, l in zip(b.centre, signs, lengths))
        for skip in (False, True):
            got = vr.brush_line(b, to, spacing, skip)
            want = spec_line(b.centre, to, spacing, skip)
            assert np.array_equal(centres(got), want), (to, spacing, skip)
            assert tuple(got[-1].centre) == to
            # consecutive dabs are at most `spacing` apart on every axis
            assert np.abs(np.diff(spec_line(b.centre, to, spacing), axis=0)).max() <= spacing
            for g in got:   # everything but the centre is the brush's
                assert (list(g.radius), g.op, g.falloff, list(g.value), list(g.strength), list(g.reserved)) == \
                       (list(b.radius), b.op, b.falloff, list(b.value), list(b.strength), [0, 0])
    # the restatement rounds halves upwards, also below zero: -7 / 2 steps -> -3.5 -> -3
    assert spec_line((0, 0, 0), (-7, 7, 0), 4)[1].tolist() == [-3, 4, 0]
    assert centres(vr.brush_line(brush((0, 0, 0)), (-7, 7, 0), 4))[1].tolist() == [-3, 4, 0]


def test_brush_line_axis_aligned_spacing_one_and_single_segment():
    import volumetricrenderer_amd as vr
    b = brush((3, 3, 3))
    got = centres(vr.brush_line(b, (3, 3, 12), 1))                     # spacing 1: every texel of the segment
    assert got.tolist() == [[3, 3, z] for z in range(3, 13)]
    got = centres(vr.brush_line(b, (-6, 3, 3), 3))                     # axis-aligned, negative
    assert got.tolist() == [[x, 3, 3] for x in (3, 0, -3, -6)]
    got = centres(vr.brush_line(b, (5, 2, 3), 50))                     # spacing above the distance: n = 1
    assert got.tolist() == [[3, 3, 3], [5, 2, 3]]
    assert centres(vr.brush_line(b, (5, 2, 3), 50, True)).tolist() == [[5, 2, 3]]
    got = centres(vr.brush_line(b, (3, 3, 3), 4))                      # no movement: n = 1, the centre twice
    assert got.tolist() == [[3, 3, 3], [3, 3, 3]]
    far = brush((-2**31, 2**31 - 1, 0))                                # the ends of int32 with a long spacing
    to = (2**31 - 1, -2**31, 5)
    got = centres(vr.brush_line(far, to, 2**22))
    assert len(got) == 1025 and np.array_equal(got, spec_line(far.centre, to, 2**22))


def test_brush_line_refusals_and_required_count():
    from volumetricrenderer_amd import _lib
    import volumetricrenderer_amd as vr
    lib = _lib.load()
    b = brush((0, 0, 0))
    to = (ctypes.c_int32 * 3)(20, -9, 3)
    out = (_lib.Brush * 8)()
    before = bytes(out)
    n = ctypes.c_int(-7)
    # max_out too small: refused, the number required reported, nothing written
    assert lib.vr_brush_line(ctypes.byref(b), to, 2, 0, out, 8, ctypes.byref(n)) == 1
    assert n.value == 11 and bytes(out) == before and "vr_brush_line:" in lib.vr_last_error().decode()
    assert lib.vr_brush_line(ctypes.byref(b), to, 2, 1, None, 0, ctypes.byref(n)) == 1 and n.value == 10
    assert lib.vr_brush_line(ctypes.byref(b), to, 3, 1, out, 8, ctypes.byref(n)) == 0 and n.value == 7
    # the n limit: 2^20 segments pass, one more is refused before anything is computed from it
    far = (ctypes.c_int32 * 3)(2**20, 0, 0)
    assert lib.vr_brush_line(ctypes.byref(b), far, 1, 0, None, 0, ctypes.byref(n)) == 1 and n.value == 2**20 + 1
    far[0] = 2**20 + 1
    assert lib.vr_brush_line(ctypes.byref(b), far, 1, 0, out, 8, ctypes.byref(n)) == 1 and n.value == 0
    assert "2^20" in lib.vr_last_error().decode()
    ends = (ctypes.c_int32 * 3)(2**31 - 1, 2**31 - 1, 2**31 - 1)
    low = brush((-2**31, -2**31, -2**31))
    assert lib.vr_brush_line(ctypes.byref(low), ends, 4095, 0, out, 8, ctypes.byref(n)) == 1 and n.value == 0
    assert lib.vr_brush_line(ctypes.byref(low), ends, 4096, 1, None, 0, ctypes.byref(n)) == 1 and n.value == 2**20
    for args in ((None, to, 1, 0, out, 8), (ctypes.byref(b), None, 1, 0, out, 8), (ctypes.byref(b), to, 1, 0, None, 8),
                 (ctypes.byref(b), to, 0, 0, out, 8), (ctypes.byref(b), to, -3, 0, out, 8), (ctypes.byref(b), to, 1, 2, out, 8),
                 (ctypes.byref(b), to, 1, 0, out, -1)):
        n.value = -7
        assert lib.vr_brush_line(*args, ctypes.byref(n)) == 1 and n.value == 0, args
    assert lib.vr_brush_line(ctypes.byref(b), to, 1, 0, out, 8, None) == 1
    bad = brush((0, 0, 0), radius=(3, 256, 4))
    assert lib.vr_brush_line(ctypes.byref(bad), to, 1, 0, out, 8, ctypes.byref(n)) == 1 and n.value == 0
    with pytest.raises(vr.VRError):
        vr.brush_line(b, (5, 5, 5), 0)
    with pytest.raises(vr.VRError):
        vr.brush_line(bad, (5, 5, 5), 1)


# ---- vr_boxes_coalesce -----------------------------------------------------------------------
def spec_coalesce(boxes, max_out):
    """include/vr.h in Python (unbounded ints): boxes are ((x, y, z), (bx, by, bz))."""
    def holds(a, b):
        return all(a[0][k] <= b[0][k] and b[1][k] <= a[1][k] for k in range(3))

    def volume(a):
        return (a[1][0] - a[0][0]) * (a[1][1] - a[0][1]) * (a[1][2] - a[0][2])

    def hull(a, b):
        return (tuple(min(a[0][k], b[0][k]) for k in range(3)), tuple(max(a[1][k], b[1][k]) for k in range(3)))

    v = []
    for o, e in boxes:
        if 0 in e:
            continue
        b = (tuple(o), tuple(o[k] + e[k] for k in range(3)))
        if any(holds(k, b) for k in v):
            continue
        v = [k for k in v if not holds(b, k)] + [b]
    while len(v) > max_out:
        best = None
        for i in range(len(v)):
            for j in range(i + 1, len(v)):
                add = volume(hull(v[i], v[j])) - volume(v[i]) - volume(v[j])
                if best is None or add < best[0]:
                    best = (add, i, j)
        _, i, j = best
        h = hull(v[i], v[j])
        v = [h if k == i else v[k] for k in range(len(v)) if k == i or (k != j and not holds(h, v[k]))]
    return [(lo, tuple(hi[k] - lo[k] for k in range(3))) for lo, hi in v]


def texels(boxes):
    out = set()
    for (x, y, z), (bx, by, bz) in boxes:
        out |= set(itertools.product(range(x, x + bx), range(y, y + by), range(z, z + bz)))
    return out


def test_coalesce_boxes_rules():
    import volumetricrenderer_amd as vr
    a, inner = ((2, 2, 2), (6, 6, 6)), ((3, 3, 3), (2, 2, 2))
    far = ((20, 20, 20), (2, 2, 2))
    assert vr.coalesce_boxes([a, inner], 8) == [a]                       # containment, either order
    assert vr.coalesce_boxes([inner, a], 8) == [a]
    assert vr.coalesce_boxes([inner, far, a], 8) == [far, a]             # what remains keeps its order
    assert vr.coalesce_boxes([a, far, a, far], 8) == [a, far]            # identical: the first is kept
    assert vr.coalesce_boxes([((1, 1, 1), (0, 5, 5)), a, ((0, 0, 0), (4, 4, 0))], 8) == [a]   # empties
    assert vr.coalesce_boxes([((1, 1, 1), (5, 0, 5))], 8) == [] and vr.coalesce_boxes([], 3) == []
    # ties go to the lowest pair of indices: four unit cubes two apart on x, every neighbouring pair adds 1
    row = [((3 * i, 0, 0), (1, 1, 1)) for i in range(4)]
    assert vr.coalesce_boxes(row, 3) == [((0, 0, 0), (4, 1, 1)), row[2], row[3]]
    # then [0, 4) with the cube at 6 adds 7 - 4 - 1 = 2, the cubes at 6 and 9 add 4 - 1 - 1 = 2: again the lowest pair
    assert vr.coalesce_boxes(row, 2) == spec_coalesce(row, 2) == [((0, 0, 0), (7, 1, 1)), row[3]]
    # max_out 1: the bounding box of the non-empty inputs
    assert vr.coalesce_boxes([a, far, ((0, 30, 1), (1, 1, 1)), ((90, 90, 90), (0, 1, 1))], 1) == [((0, 2, 1), (22, 29, 21))]
    # the merged box goes to the place of the pair's first, and swallows what it contains
    lst = [((0, 0, 0), (2, 2, 2)), ((50, 0, 0), (1, 1, 1)), ((3, 3, 3), (2, 2, 2)), ((1, 1, 1), (3, 3, 1))]
    assert vr.coalesce_boxes(lst, 2) == spec_coalesce(lst, 2) == [((0, 0, 0), (5, 5, 5)), ((50, 0, 0), (1, 1, 1))]
    # coordinates at the end of int32: volumes beyond 64 bits
    big = 2**31 - 1
    huge = [((0, 0, 0), (big, big, big)), ((5, 5, 5), (1, 1, 1))]
    assert vr.coalesce_boxes(huge, 4) == [huge[0]]
    corners = [((0, 0, 0), (1, 1, 1)), ((big - 1, big - 1, big - 1), (1, 1, 1)), ((big - 1, 0, 0), (1, 1, 1))]
    assert vr.coalesce_boxes(corners, 2) == spec_coalesce(corners, 2) == [((0, 0, 0), (big, 1, 1)), corners[1]]


def test_coalesce_boxes_matches_restatement_and_covers():
    import volumetricrenderer_amd as vr
    rng = np.random.default_rng(20240627)
    merged = 0
    for it in range(300):
        dim = int(rng.integers(4, 40))
        count = int(rng.integers(0, 70 if it % 10 == 0 else 14))     # now and then past VR_MAX_DABS (the heap path)
        boxes = []
        for _ in range(count):
            e = [int(rng.integers(0 if rng.integers(0, 8) == 0 else 1, min(dim, 9) + 1)) for _ in range(3)]
            boxes.append((tuple(int(rng.integers(0, dim - e[k] + 1)) for k in range(3)), tuple(e)))
        if count > 2:
            boxes[int(rng.integers(0, count))] = boxes[int(rng.integers(0, count))]
        max_out = int(rng.integers(1, 10))
        got = vr.coalesce_boxes(boxes, max_out)
        assert got == spec_coalesce(boxes, max_out), (it, boxes, max_out)
        assert len(got) <= max_out
        assert texels(boxes) <= texels(got)          # every input texel is inside some output box
        merged += len(spec_coalesce(boxes, 10**6)) > max_out
    assert merged > 100
    # the stroke's case: 64 overlapping cubes along a diagonal in 8 boxes, far below the bounding box
    run = [((4 * i, 4 * i, 4 * i), (17, 17, 17)) for i in range(64)]
    got = vr.coalesce_boxes(run, 8)
    assert got == spec_coalesce(run, 8) and len(got) == 8
    assert sum(e[0] * e[1] * e[2] for _, e in got) < 269**3 // 8


def test_coalesce_boxes_refusals():
    from volumetricrenderer_amd import _lib
    import volumetricrenderer_amd as vr
    lib = _lib.load()
    good = ((1, 1, 1), (2, 2, 2))
    big = 2**31 - 1
    for bad in (((-1, 0, 0), (1, 1, 1)), ((0, 0, -4), (1, 1, 1)), ((0, 0, 0), (1, -1, 1)), ((big, 0, 0), (1, 1, 1)),
                ((0, 7, 0), (1, big - 6, 1)), ((0, 0, 1), (1, 1, big))):
        with pytest.raises(vr.VRError) as e:
            vr.coalesce_boxes([good, bad, good], 4)
        assert e.value.status == 1 and "box 1" in str(e.value)
    for max_out in (0, -2):
        with pytest.raises(vr.VRError):
            vr.coalesce_boxes([good], max_out)
    one, out, n = _lib.Box(0, 0, 0, 1, 1, 1), _lib.Box(), ctypes.c_int(-7)
    assert lib.vr_boxes_coalesce(None, 1, 1, ctypes.byref(out), ctypes.byref(n)) == 1
    assert lib.vr_boxes_coalesce(ctypes.byref(one), 1, 1, None, ctypes.byref(n)) == 1
    assert lib.vr_boxes_coalesce(ctypes.byref(one), 1, 1, ctypes.byref(out), None) == 1
    assert lib.vr_boxes_coalesce(ctypes.byref(one), -1, 1, ctypes.byref(out), ctypes.byref(n)) == 1 and n.value == -7
    assert "vr_boxes_coalesce:" in lib.vr_last_error().decode()
    assert lib.vr_boxes_coalesce(None, 0, 1, None, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.vr_boxes_coalesce(None, 0, 1, None, None) == 0


# ---- layout, prototypes, exports, argument checks -------------------------------------------
def header_source():
    src = open(os.path.join(ROOT, "include", "vr.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_box_layout_in_header_ctypes_and_hpp(tmp_path):
    from volumetricrenderer_amd import _lib
    import volumetricrenderer_amd as vr
    fields = ("x", "y", "z", "bx", "by", "bz")
    assert ctypes.sizeof(_lib.Box) == 24
    assert [getattr(_lib.Box, f).offset for f in fields] == [0, 4, 8, 12, 16, 20]
    assert vr.VR_MAX_DABS == _lib.VR_MAX_DABS == 64 and vr.Box is _lib.Box
    offs = ", ".join(f"offsetof(vr_box, {f})" for f in fields)
    body = (f'int main(void){{printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(vr_box), {offs}, (int)VR_MAX_DABS); '
            "return 0;}\n")
    c = tmp_path / "box.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vr.h"\n' + body)
    cpp = tmp_path / "box.cpp"   # the C++ wrapper: PaintStroke and BrushLine exist
    cpp.write_text('#include <cstdio>\n#include <cstddef>\n#include "vr_renderer.hpp"\n'
                   "void (vr::Renderer::*stroke_fn)(const vr_brush*, int, void*) = &vr::Renderer::PaintStroke;\n"
                   "void (vr::Renderer::*stroke_vec_fn)(const std::vector<vr_brush>&, void*) = &vr::Renderer::PaintStroke;\n"
                   "std::vector<vr_brush> (*line_fn)(const vr_brush&, const int32_t*, int, bool) = &vr::BrushLine;\n"
                   + body)
    for src, cc, std in ((c, "gcc", "-std=c99"), (cpp, "g++", "-std=c++17")):
        exe = tmp_path / (src.name + ".exe")
        libdir = os.path.join(ROOT, "volumetricrenderer_amd")
        subprocess.run([cc, std, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lvr",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
        got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
        assert got == [24, 0, 4, 8, 12, 16, 20, 64], (cc, got)


def test_prototypes_exports_and_signatures():
    from volumetricrenderer_amd import _lib
    import volumetricrenderer_amd as vr
    lib = _lib.load()
    src = header_source()
    declared = set(re.findall(r"\b(vr_[a-z_0-9]+)\s*\(", src))
    for name, nargs in zip(NEW, (4, 7, 5)):
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
        m = re.search(r"vr_status\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib._SIGS[name][1]), name
        assert _lib._SIGS[name][0] is ctypes.c_int
    assert re.search(r"vr_status\s+vr_paint_stroke\s*\(\s*void\*\s*ctx,\s*const vr_brush\*\s*dabs,\s*int count,\s*void\*\s*stream\)",
                     src)
    assert re.search(r"#define\s+VR_MAX_DABS\s+64\b", src)
    assert lib.vr_abi_version() == 2
    for name in ("brush_line", "coalesce_boxes", "VR_MAX_DABS"):
        assert name in vr.__all__ and hasattr(vr, name)
    assert callable(vr.Renderer.paint_stroke)


def test_paint_stroke_argument_checks_come_before_the_context():
    """Every refusal that needs no context is made before the context is read (a dangling handle is never touched)."""
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    dabs = (_lib.Brush * 5)(*[brush((i, i, i)) for i in range(5)])
    ctx = ctypes.c_void_p(8)
    assert lib.vr_paint_stroke(None, dabs, 5, None) == 1 and "null" in lib.vr_last_error().decode()
    assert lib.vr_paint_stroke(None, None, 0, None) == 1
    for count in (-1, -2**31, 65, 2**31 - 1):
        assert lib.vr_paint_stroke(ctx, dabs, count, None) == 1
        assert "vr_paint_stroke:" in lib.vr_last_error().decode() and "count" in lib.vr_last_error().decode()
    assert lib.vr_paint_stroke(ctx, None, 1, None) == 1 and "null" in lib.vr_last_error().decode()
    assert lib.vr_paint_stroke(ctx, None, 0, None) == 0        # count 0: VR_OK, nothing read
    dabs[3].op = 7
    assert lib.vr_paint_stroke(ctx, dabs, 5, None) == 1
    assert "dab 3" in lib.vr_last_error().decode() and "bad op" in lib.vr_last_error().decode()
