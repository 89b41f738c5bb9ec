"""vr_paint_stroke on the GPU: after a stroke the volume is, byte for byte, what
the CPU loop of vr_brush_apply over the same dabs leaves (tests/paint_spec.py
is the reference for vr_brush_apply itself, tests/test_paint_cpu.py); the
painted context's frame and step counter against a fresh install of the
CPU-painted volume and against the CPU oracle, per layout; a second context
that received the same dabs as separate vr_paint calls; uniform channels;
stream order; refusals.  Everything is exact.

Volume A is the 37 x 22 x 45 of the paint tests (no axis a multiple of a brick
edge), volume B is 150 x 9 x 7, whose rows exceed a wave's 64 lanes.  Frames
are brush_harness.py's: the reference camera at 64 x 64, 32 steps.  Each case
also asserts, on the CPU side, the condition that makes its input a test of
what it names (order dependence, overlap depth, the clamp, ...).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paint_spec as ps  # noqa: E402
from brush_harness import (H, LAYOUT_IDS, LAYOUTS, W, assert_exact, assert_marches, base, check_frame,  # noqa: E402,F401
                           check_fresh_install, check_needs_a_volume, frame, fresh, oracle_frame, r, recipe_volume, setup)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd import _lib  # noqa: E402
from volumetricrenderer_amd._lib import FMT_RGBA32F  # noqa: E402

NX, NY, NZ = ps.NX, ps.NY, ps.NZ
BX, BY, BZ = 150, 9, 7
UNIFORM_VARIANTS = {12, 14, 15}   # the layouts whose march has the _uX (no loads for one channel) kernels


def cpu_stroke(vol, dabs):
    """The reference: vr_brush_apply of every dab in order on a copy of `vol`."""
    out = vol.copy()
    for b in dabs:
        vr.brush_apply(b, out)
    return out


def coverage(shape, dabs):
    """How many of the dabs' ellipsoids hold each texel (the numpy restatement's inside masks)."""
    n = np.zeros(shape[:3], np.int32)
    for b in dabs:
        n += ps.spec_weights(shape[:3], tuple(b.centre), tuple(b.radius), b.falloff)[0]
    return n


@pytest.fixture(scope="module")
def long_base():
    return np.random.default_rng(ps.SEED + 1).integers(0, 256, size=(BZ, BY, BX, 4), dtype=np.uint8)


@pytest.fixture(scope="module")
def heavy(base):
    """Stroke 2: 64 smooth dabs of radius 5, spacing 2, forth (SET), back (ADD) and forth again (SUB) along A's
    diagonal, strengths (255, 128, 0, 64) -- and the volume the CPU loop leaves."""
    a, z = (0, 0, 0), (NX - 1, NY - 1, NZ - 1)
    strength = (255, 128, 0, 64)
    dabs = vr.brush_line(vr.make_brush(a, 5, ps.SET, 1, ps.VALUE, strength), z, 2)
    dabs += vr.brush_line(vr.make_brush(z, 5, ps.ADD, 1, (90, 70, 50, 30), strength), a, 2, skip_first=True)
    dabs += vr.brush_line(vr.make_brush(a, 5, ps.SUB, 1, (60, 200, 9, 120), strength), z, 2, skip_first=True)
    dabs = dabs[:vr.VR_MAX_DABS]
    assert len(dabs) == 64 and {b.op for b in dabs} == {ps.SET, ps.ADD, ps.SUB}
    painted = cpu_stroke(base, dabs)
    assert coverage(base.shape, dabs).max() >= 4, "no texel is covered by four dabs"
    assert (painted[..., 2] == base[..., 2]).all() and (painted[..., :2] != base[..., :2]).any()
    return dabs, painted


def stroke_equals_cpu(rr, vol, dabs, dims=(NX, NY, NZ)):
    """Install `vol`, paint the stroke, compare with the CPU loop; returns the painted volume."""
    rr.set_layout_preference(14)
    rr.set_volume(vol)
    boxes = rr.paint_stroke(dabs)
    assert boxes == [b for b in (vr.brush_box(d, dims) for d in dabs) if b is not None]
    want = cpu_stroke(vol, dabs)
    assert_exact(rr.get_volume(), want)
    return want


# ---- 1. order matters ------------------------------------------------------------------------
def test_order_matters(r, base):
    s = vr.make_brush((17, 11, 23), (6, 5, 7), ps.SET, 1, (200,) * 4, (255,) * 4)
    a = vr.make_brush((20, 12, 25), (6, 5, 7), ps.ADD, 0, (40,) * 4, (255,) * 4)
    assert coverage(base.shape, [s, a]).max() == 2, "the dabs do not overlap"
    one, two = cpu_stroke(base, [s, a]), cpu_stroke(base, [a, s])
    assert (one != two).any(), "SET then ADD equals ADD then SET on this input"
    assert_exact(stroke_equals_cpu(r, base, [s, a]), one)
    assert_exact(stroke_equals_cpu(r, base, [a, s]), two)


# ---- 2. heavy overlap ------------------------------------------------------------------------
def test_heavy_overlap(r, base, heavy):
    dabs, painted = heavy
    assert_exact(stroke_equals_cpu(r, base, dabs), painted)


# ---- 3. the same ADD dab three times ---------------------------------------------------------
def test_same_add_dab_three_times(r, base):
    b = vr.make_brush((18, 11, 22), (7, 6, 8), ps.ADD, 1, (100, 100, 100, 100), (255, 255, 255, 255))
    want = cpu_stroke(base, [b, b, b])
    twice = cpu_stroke(base, [b, b])
    assert ((want == 255) & (twice < 255)).any(), "the third dab never reaches the clamp at 255"
    assert ((want < 255) & (want != base)).any(), "every painted texel clamps"
    assert_exact(stroke_equals_cpu(r, base, [b, b, b]), want)


# ---- 4. a mixed list -------------------------------------------------------------------------
@pytest.mark.parametrize("whole_at", ["first", "last"])
def test_mixed_list(r, base, whole_at):
    whole = vr.make_brush(*ps.BRUSHES["whole"], ps.SET, 1, ps.VALUE, (200, 128, 1, 90))
    assert vr.brush_box(whole, (NX, NY, NZ)) == ((0, 0, 0), (NX, NY, NZ))
    dabs = [
        vr.make_brush((17, 11, 23), 0, ps.SET, 0, (1, 2, 3, 4), (255,) * 4),                  # radius 0, twice on a texel
        vr.make_brush((17, 11, 23), 0, ps.ADD, 1, (9, 9, 9, 9), (255, 0, 255, 128)),
        vr.make_brush(*ps.BRUSHES["outside_centre"], ps.SUB, 1, ps.VALUE, ps.STRENGTH),       # centred outside, reaches in
        vr.make_brush(*ps.BRUSHES["straddle"], ps.ADD, 0, ps.VALUE, (255, 128, 1, 0)),
        vr.make_brush(*ps.BRUSHES["miss"], ps.SET, 0, ps.VALUE, ps.STRENGTH),                 # misses, mid-list
        vr.make_brush(*ps.BRUSHES["corner"], ps.SUB, 0, (30, 250, 70, 255), (255,) * 4),
        vr.make_brush(*ps.BRUSHES["far_corner"], ps.SET, 1, ps.VALUE, (255, 255, 0, 3)),
        vr.make_brush(*ps.BRUSHES["interior"], ps.ADD, 1, ps.VALUE, ps.STRENGTH),
        vr.make_brush((0, 21, 0), 0, ps.SUB, 0, (255,) * 4, (255,) * 4),                      # radius 0 in a corner
    ]
    dabs = [whole] + dabs if whole_at == "first" else dabs + [whole]
    assert {(b.op, b.falloff) for b in dabs} == {(o, f) for o in (0, 1, 2) for f in (0, 1)}
    assert vr.brush_box(dabs[5 if whole_at == "first" else 4], (NX, NY, NZ)) is None
    assert vr.brush_box(dabs[3 if whole_at == "first" else 2], (NX, NY, NZ)) is not None
    want = stroke_equals_cpu(r, base, dabs)
    assert (want != cpu_stroke(base, dabs[::-1])).any()
    assert len(r.paint_stroke(dabs)) == len(dabs) - 1   # the miss is dropped from the boxes too


# ---- 5. rows longer than a wave --------------------------------------------------------------
def test_long_rows(r, long_base):
    ops = [(ps.SET, 1), (ps.ADD, 0), (ps.SUB, 1)]
    dabs = [vr.make_brush((40 + 35 * i, 4, 3), (70, 3, 2), op, f, (200 - 60 * i, 60, 255, 10), (255, 128, 64, 255))
            for i, (op, f) in enumerate(ops)]
    boxes = [vr.brush_box(b, (BX, BY, BZ)) for b in dabs]
    assert max(e[0] for _, e in boxes) > 128, "no clipped box is wider than two waves"
    assert coverage(long_base.shape, dabs).max() == 3
    want = stroke_equals_cpu(r, long_base, dabs, (BX, BY, BZ))
    assert (want != long_base).any()


# ---- 6. count 1, count 0, all misses ---------------------------------------------------------
def test_count_one_zero_and_all_misses(r, fresh, base):
    b = vr.make_brush(*ps.BRUSHES["straddle"], ps.SET, 1, ps.VALUE, ps.STRENGTH)
    stroke_equals_cpu(r, base, [b])
    fresh.set_layout_preference(14)
    fresh.set_volume(base)
    fresh.paint(*ps.BRUSHES["straddle"], ps.SET, 1, ps.VALUE, ps.STRENGTH)
    assert_exact(r.get_volume(), fresh.get_volume())
    r.set_volume(base)
    assert r.paint_stroke([]) == []
    _lib.call("vr_paint_stroke", r._ctx, None, 0, None)            # dabs may be NULL with count 0
    misses = [vr.make_brush(*ps.BRUSHES["miss"]), vr.make_brush((2**31 - 1, 5, 5), 255), vr.make_brush((5, -2**31, 5), 255),
              vr.make_brush((NX + 4, 5, 5), (4, 9, 9))]
    assert all(vr.brush_box(m, (NX, NY, NZ)) is None for m in misses)
    assert r.paint_stroke(misses) == []
    assert_exact(r.get_volume(), base)
    setup(fresh, 14, base)          # an all-miss stroke leaves a rendering context as it is
    setup(r, 14, base)
    assert r.paint_stroke(misses) == []
    img, steps = frame(r)
    img2, steps2 = frame(fresh)
    assert_exact(img, img2)
    assert steps == steps2


# ---- 7. per layout: the frame, the oracle, and the same dabs as separate paints --------------
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_stroke_render_per_layout(r, fresh, oracle, base, heavy, pref, lname):
    dabs, painted = heavy
    ref, ref_steps = oracle_frame(oracle, painted)
    before, _ = oracle_frame(oracle, base)
    assert (ref != before).any(), "the stroke does not change the oracle's frame"
    setup(r, pref, base)
    assert_marches(r, lname)
    pre, _ = frame(r)
    assert_exact(pre, before)
    r.paint_stroke(dabs)
    assert_marches(r, lname)
    img, steps = check_frame(r, oracle, painted)
    setup(fresh, pref, base)          # the same dabs as 64 vr_paint calls on a second context
    for b in dabs:
        _lib.call("vr_paint", fresh._ctx, ctypes.byref(b), None)
    torch.cuda.synchronize()
    assert_exact(fresh.get_volume(), r.get_volume())
    img3, steps3 = frame(fresh)
    assert_exact(img3, img)
    assert steps3 == steps
    check_fresh_install(fresh, pref, lname, painted, img, steps)   # the CPU-painted volume


# ---- 8. uniform channels on the recipe volume ------------------------------------------------


@pytest.mark.parametrize("case", ["strength0", "changed", "undone"])
@pytest.mark.parametrize("pref,lname", [(0, "auto"), (12, "brick4832"), (15, "col48")], ids=["auto", "brick4832", "col48"])
def test_uniform_channel(r, oracle, recipe_volume, pref, lname, case):
    vol, g = recipe_volume
    d = 37
    first, second = (ps.ADD, ps.SUB) if g + d <= 255 else (ps.SUB, ps.ADD)
    line = lambda op, falloff, value, strength: vr.brush_line(  # noqa: E731
        vr.make_brush((6, 7, 8), (5, 4, 6), op, falloff, value, strength), (25, 22, 20), 3)
    if case == "strength0":      # a. G is left alone
        dabs, keeps = line(ps.SET, 1, (200, 200, 255, 10), (255, 0, 255, 128)), True
    elif case == "changed":      # b. G is changed
        dabs, keeps = line(ps.SET, 1, (200, (g + 100) % 256, 255, 10), (255, 255, 0, 128)), False
    else:                        # c. a hard ADD of d on G and the identical SUB (or the reverse): every G byte returns to g
        fwd = line(first, 0, (9, d, 9, 9), (255, 255, 0, 0))[:8]
        dabs = [x for b in fwd for x in (b, vr.make_brush(tuple(b.centre), tuple(b.radius), second, 0, (9, d, 9, 9),
                                                         (255, 255, 0, 0)))]
        keeps = True
        half = cpu_stroke(vol, dabs[:1])
        assert (half[..., 1] != g).any(), "the first dab does not change G"
    assert 1 < len(dabs) <= vr.VR_MAX_DABS
    painted = cpu_stroke(vol, dabs)
    assert ((painted[..., 1] == g).all()) == keeps
    assert (painted != vol).any() or case == "undone"
    setup(r, pref, vol)
    assert r.get_option("uniform_mask") & 2
    uses_u = r.kernel_variant.endswith("_uG")
    assert uses_u or pref not in UNIFORM_VARIANTS
    r.paint_stroke(dabs)
    assert bool(r.get_option("uniform_mask") & 2) == keeps
    assert r.kernel_variant.endswith("_uG") == (keeps and uses_u)
    check_frame(r, oracle, painted)


# ---- 9. stroke and render_rects on a side stream, no host sync -------------------------------
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_stroke_then_render_rects_on_a_side_stream(r, oracle, base, heavy, pref, lname):
    dabs, painted = heavy
    setup(r, pref, base)
    assert_marches(r, lname)
    buf = r.render(W, H, FMT_RGBA32F)
    torch.cuda.synchronize()
    assert_exact(buf.cpu().numpy(), oracle_frame(oracle, base)[0])
    s = torch.cuda.Stream()
    boxes = r.paint_stroke(dabs, stream=s)
    rects = r.update_footprints(boxes, W, H)        # host arithmetic
    assert len(rects) == len(dabs)
    r.render_rects(buf, rects, FMT_RGBA32F, stream=s)
    s.synchronize()
    assert_exact(buf.cpu().numpy(), oracle_frame(oracle, painted)[0])
    assert_exact(r.get_volume(), painted)


# ---- 10. refusals ----------------------------------------------------------------------------
def test_refusals(r, base):
    setup(r, 0, base)
    good = [vr.make_brush((10 + i, 11, 20), (3, 2, 4), ps.ADD, 1, ps.VALUE, ps.STRENGTH) for i in range(5)]
    assert (cpu_stroke(base, good[:3]) != base).any()

    def refused(status, *args, needle="vr_paint_stroke"):
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_paint_stroke", *args)
        assert e.value.status == status and needle in str(e.value), str(e.value)
        assert np.array_equal(r.get_volume(), base)

    many = (_lib.Brush * 65)(*[good[0]] * 65)
    arr = (_lib.Brush * 5)(*good)
    refused(1, r._ctx, many, 65, None, needle="count 65")
    with pytest.raises(vr.VRError):
        r.paint_stroke([good[0]] * 65)
    refused(1, r._ctx, arr, -1, None, needle="count -1")
    refused(1, r._ctx, None, 1, None, needle="null")
    for field, value in (("op", 3), ("falloff", 2), ("radius", 256), ("reserved", 1)):
        bad = (_lib.Brush * 5)(*good)
        if field in ("op", "falloff"):
            setattr(bad[3], field, value)
        else:
            getattr(bad[3], field)[1] = value
        refused(1, r._ctx, bad, 5, None, needle="dab 3")      # the three valid dabs before it were not applied
    _lib.call("vr_paint_stroke", r._ctx, many, 64, None)       # 64 is accepted
    torch.cuda.synchronize()
    assert_exact(r.get_volume(), cpu_stroke(base, [good[0]] * 64))
    r.set_volume(base)
    check_needs_a_volume(r, lambda rr: rr.paint_stroke(good))
    assert np.array_equal(r.get_volume(), base)
