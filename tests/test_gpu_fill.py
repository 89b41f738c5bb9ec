"""vr_fill on the GPU: the filled volume and the device report against the numpy
restatement (tests/fill_spec.py), byte for byte, on every volume x brush x op x
falloff x relative / absolute; all strengths 0 with a report; seeds on a tile
corner, in the last partial tile of each axis and outside the ellipsoid; the
larger volume; the edited context's frame against a fresh install of the
specification's volume and against the CPU oracle, per layout; a fill and a
render_rect queued on one side stream; uniform channels; the scratch it shares
with vr_blur; undo; refusals.  Everything is exact.

Frame, march and cameras are brush_harness.py's: the reference camera at
64 x 64, 32 steps.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blur_spec as bs  # noqa: E402
import fill_spec as fs  # noqa: E402
import paint_spec as ps  # noqa: E402
from brush_harness import (H, LAYOUT_IDS, LAYOUTS, UNIFORM_LAYOUTS, W, assert_exact, assert_marches, check_frame,  # noqa: E402,F401
                           check_fresh_install, check_needs_a_volume, frame, fresh, oracle_frame, r, recipe_volume, setup)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd import _lib  # noqa: E402
from volumetricrenderer_amd._lib import FMT_RGBA32F  # noqa: E402

NX, NY, NZ = ps.NX, ps.NY, ps.NZ
DIMS = (NX, NY, NZ)
CASES = ["blobs", "snakes", "detour", "edges"]


@pytest.fixture(scope="module")
def cases():
    return fs.cases()


def lib_rule(rule):
    return vr.make_fill_rule(rule.seed, rule.lo, rule.hi, rule.select, rule.relative)


def fill(rr, centre, radius, op, falloff, rule, strength=fs.STRENGTH, report=True, stream=None):
    """((origin, extent), the report as a tuple) of a vr_fill with the shared value."""
    out = rr.fill(None, centre, radius, op, falloff, fs.VALUE, strength, rule=lib_rule(rule), report=report, stream=stream)
    if report is None:
        return out, None
    return out[0], tuple(vr.unpack_fill_report(out[1]))


def rule_of(cases, cname, centre, relative, channel=None):
    case = cases[cname]
    if cname == "edges":
        return fs.edge_rule(case.vol, case.seed(centre))
    return case.rule(centre, relative, channel)


# ---- 1. the filled volume and the report are the specification's ------------------------------
@pytest.mark.parametrize("relative", [0, 1], ids=["absolute", "relative"])
@pytest.mark.parametrize("name", list(ps.BRUSHES))
@pytest.mark.parametrize("cname", CASES)
def test_filled_volume_and_report_equal_the_specification(r, cases, cname, name, relative):
    vol = cases[cname].vol
    centre, radius = ps.BRUSHES[name]
    rule = rule_of(cases, cname, centre, relative)
    r.set_layout_preference(14)
    for op, _ in ps.OPS:
        for falloff, _ in ps.FALLOFFS:
            r.set_volume(vol)
            want, want_rep = fs.spec_fill(vol, centre, radius, op, falloff, rule)
            box, rep = fill(r, centre, radius, op, falloff, rule)
            assert box == ps.spec_box(centre, radius)
            assert rep == want_rep
            assert_exact(r.get_volume(), want)
    if name in ("whole", "max"):
        assert want_rep[0] > 0 and (want != vol).any()
    # all strengths 0 with a report: a measurement -- the report exact, the volume as it was
    r.set_volume(vol)
    box, rep = fill(r, centre, radius, ps.SET, 0, rule, strength=(0, 0, 0, 0))
    assert rep == want_rep
    assert_exact(r.get_volume(), vol)
    # and without a report the painted volume is the same
    r.set_volume(vol)
    box, rep = fill(r, centre, radius, ps.ADD, 1, rule, report=None)
    assert box == ps.spec_box(centre, radius) and rep is None
    assert_exact(r.get_volume(), fs.spec_fill(vol, centre, radius, ps.ADD, 1, rule)[0])


@pytest.mark.parametrize("cname", ["blobs", "snakes", "detour"])
def test_the_selected_channel_need_not_be_painted(r, cases, cname):
    vol = cases[cname].vol
    centre, radius = ps.BRUSHES["whole"]
    r.set_layout_preference(0)
    for relative in (0, 1):
        on_a = rule_of(cases, cname, centre, relative, 3)
        on_r = rule_of(cases, cname, centre, relative, 0)
        both = fs.Rule(on_r.seed, (on_r.lo[0], 0, 0, on_a.lo[3]), (on_r.hi[0], 0, 0, on_a.hi[3]), (1, 0, 0, 1), relative)
        for rule, strength in ((on_a, fs.STRENGTH), (both, (0, 255, 0, 0))):
            r.set_volume(vol)
            want, want_rep = fs.spec_fill(vol, centre, radius, ps.SUB, 1, rule, strength=strength)
            box, rep = fill(r, centre, radius, ps.SUB, 1, rule, strength)
            assert rep == want_rep and rep[0] > 0 and (want != vol).any()
            assert_exact(r.get_volume(), want)


# ---- 2. seeds ---------------------------------------------------------------------------------
def test_each_corridor_from_seeds_on_tile_corners_and_in_the_last_tiles(r):
    """The corridors' texels on a tile corner (every coordinate a multiple of 8) and in the last, partial tile of
    each axis (x >= 32, y >= 16, z >= 40) as seeds: each fills its own corridor and nothing of the other."""
    vol, a, b = fs.snakes()
    centre, radius = ps.BRUSHES["whole"]
    r.set_layout_preference(0)
    used = 0
    for path in (a, b):
        picks = [next(t for t in path if all(v % 8 == 0 for v in t)),
                 next(t for t in path if t[0] >= 32), next(t for t in path if t[1] >= 16), next(t for t in path if t[2] >= 40),
                 next(t for t in path if t[0] >= 32 and t[1] >= 16 and t[2] >= 40)]
        for seed in picks:
            rule = fs.relative_rule(vol, seed, fs.SNAKE_LO, fs.SNAKE_HI)
            r.set_volume(vol)
            want, want_rep = fs.spec_fill(vol, centre, radius, ps.SET, 0, rule, strength=fs.FULL)
            box, rep = fill(r, centre, radius, ps.SET, 0, rule, fs.FULL)
            assert rep == want_rep and rep[0] == len(path) and rep[1] == len(a) + len(b)
            assert_exact(r.get_volume(), want)
            used += 1
    assert used == 10


def test_a_seed_outside_the_ellipsoid_fills_nothing(r, cases):
    vol = cases["blobs"].vol
    centre, radius = (18, 11, 22), (10, 8, 12)
    corner = (8, 3, 10)                                   # inside the clipped box, outside the ellipsoid
    inside, _ = ps.spec_weights(vol.shape[:3], centre, radius, 0)
    assert not inside[corner[2], corner[1], corner[0]]
    every = fs.Rule(corner, (255, 0, 0, 0), (255, 0, 0, 0), (1, 0, 0, 0), 1)
    r.set_layout_preference(0)
    r.set_volume(vol)
    box, rep = fill(r, centre, radius, ps.SET, 0, every, fs.FULL)
    assert rep == (0, int(inside.sum()), DIMS, (-1, -1, -1))
    assert_exact(r.get_volume(), vol)
    box, rep = fill(r, centre, radius, ps.SET, 0, every._replace(seed=(0, 0, 0)), fs.FULL)   # outside the clipped box
    assert rep == fs.empty_report(DIMS)
    assert_exact(r.get_volume(), vol)
    # a texel brush on its own seed fills that texel
    seed = cases["blobs"].seed((17, 11, 23))
    rule = cases["blobs"].rule((17, 11, 23), 1)
    box, rep = fill(r, seed, (0, 0, 0), ps.SET, 0, rule, fs.FULL)
    assert box == (seed, (1, 1, 1)) and rep == (1, 1, seed, seed)
    assert_exact(r.get_volume(), fs.spec_fill(vol, seed, (0, 0, 0), ps.SET, 0, rule, strength=fs.FULL)[0])


# ---- 3. the larger volume: labels past 16 bits ------------------------------------------------
def test_the_larger_volume():
    vol, a, b = fs.snakes(fs.LARGE)
    nx, ny, nz = fs.LARGE
    assert nx * ny * nz == 94710 > 65536
    centre, radius = (nx // 2, ny // 2, nz // 2), (255, 255, 255)
    seed = b[-1]                                          # the far end: the last z plane
    assert seed[2] == nz - 1 and (seed[2] * ny + seed[1]) * nx + seed[0] > 65536
    rule = fs.relative_rule(vol, seed, fs.SNAKE_LO, fs.SNAKE_HI)
    want, want_rep = fs.spec_fill(vol, centre, radius, ps.SET, 1, rule, strength=fs.FULL)
    assert want_rep[0] == len(b) and want_rep[1] == len(a) + len(b)
    with vr.Renderer(0) as rr:
        rr.set_volume(vol)
        box, rep = fill(rr, centre, radius, ps.SET, 1, rule, fs.FULL)
        assert box == ((0, 0, 0), fs.LARGE) and rep == want_rep
        assert_exact(rr.get_volume(), want)


# ---- 4. the edited context renders what a fresh install of the specification's volume renders --
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_filled_render_equals_fresh_install(r, fresh, oracle, cases, pref, lname):
    vol = cases["blobs"].vol
    setup(r, pref, vol)
    assert_marches(r, lname)
    for name, op in (("straddle", ps.SET), ("whole", ps.ADD)):
        centre, radius = ps.BRUSHES[name]
        rule = cases["blobs"].rule(centre, 1)
        before, _ = oracle_frame(oracle, vol)
        vol, want_rep = fs.spec_fill(vol, centre, radius, op, 1, rule, strength=fs.FULL)
        assert want_rep[0] > 0
        ref, ref_steps = oracle_frame(oracle, vol)
        assert (ref != before).any(), "the fill does not change the oracle's frame"
        box, rep = fill(r, centre, radius, op, 1, rule, fs.FULL)
        assert rep == want_rep
        assert_marches(r, lname)
        img, steps = check_frame(r, oracle, vol)
        check_fresh_install(fresh, pref, lname, vol, img, steps)


# ---- 5. one stream, no host wait ---------------------------------------------------------------
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_a_fill_then_render_rect_on_a_side_stream(r, oracle, cases, pref, lname):
    """A fill under `whole`, its footprint and the re-render of that rectangle queue on one side stream with one
    synchronise at the end."""
    base = cases["blobs"].vol
    setup(r, pref, base)
    assert_marches(r, lname)
    buf = r.render(W, H, FMT_RGBA32F)
    centre, radius = ps.BRUSHES["whole"]
    rule = cases["blobs"].rule(centre, 1)
    report = torch.zeros(vr.FILL_REPORT_BYTES, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    (origin, extent), out = r.fill(None, centre, radius, ps.SET, 1, fs.VALUE, fs.FULL, rule=lib_rule(rule), report=report, stream=s)
    assert out is report
    rect = r.update_footprint(origin, extent, W, H)
    r.render_rect(buf, rect, FMT_RGBA32F, stream=s)
    s.synchronize()
    once, want_rep = fs.spec_fill(base, centre, radius, ps.SET, 1, rule, strength=fs.FULL)
    assert tuple(vr.unpack_fill_report(report)) == want_rep
    assert_exact(r.get_volume(), once)
    want, want_steps = oracle_frame(oracle, once)
    assert (want != oracle_frame(oracle, base)[0]).any()
    assert_exact(buf.cpu().numpy(), want)
    img, steps = frame(r)
    assert_exact(img, want)
    assert steps == want_steps


# ---- 6. uniform channels on the recipe volume --------------------------------------------------


@pytest.mark.parametrize("pref,lname", UNIFORM_LAYOUTS, ids=[n for _, n in UNIFORM_LAYOUTS])
def test_uniform_channel(r, fresh, oracle, recipe_volume, pref, lname):
    vol, g = recipe_volume
    centre, radius = (15, 17, 14), (12, 10, 13)
    seed = centre
    rule = fs.Rule(seed, (40, 0, 0, 0), (40, 0, 0, 0), (1, 0, 0, 0), 1)
    setup(r, pref, vol)
    assert r.get_option("uniform_mask") & 2 and r.kernel_variant.endswith("_uG")
    # a SET fill to G's own value on every channel's strength: G keeps its bit
    value = (200, g, 60, 255)
    r.fill(seed, centre, radius, ps.SET, 1, value, fs.FULL, rule=lib_rule(rule))
    kept, rep = fs.spec_fill(vol, centre, radius, ps.SET, 1, rule, value=value, strength=fs.FULL)
    assert rep[0] > 1 and (kept != vol).any() and (kept[..., 1] == g).all()
    assert r.get_option("uniform_mask") & 2 and r.kernel_variant.endswith("_uG")
    check_frame(r, oracle, kept)
    # one that changes a byte of G loses it before the next render
    value = (200, (g + 90) % 256, 60, 255)
    rule2 = fs.Rule(seed, (255, 0, 0, 0), (255, 0, 0, 0), (1, 0, 0, 0), 1)
    r.fill(seed, centre, radius, ps.SET, 0, value, (0, 255, 0, 0), rule=lib_rule(rule2))
    lost, rep = fs.spec_fill(kept, centre, radius, ps.SET, 0, rule2, value=value, strength=(0, 255, 0, 0))
    assert rep[0] > 1 and (lost[..., 1] != g).any()
    assert not r.get_option("uniform_mask") & 2
    img, steps = frame(r)
    ref, ref_steps = oracle_frame(oracle, lost)
    assert_exact(img, ref)
    assert steps == ref_steps
    setup(fresh, pref, lost)
    img2, steps2 = frame(fresh)
    assert_exact(img, img2)
    assert steps == steps2


# ---- 7. the labels live in the blur's scratch --------------------------------------------------
def test_scratch_is_shared_with_blur(cases):
    base = cases["blobs"].vol
    with vr.Renderer(0) as rr:
        assert rr.get_option("blur_scratch_kib") == 0
        rr.set_volume(base)
        centre, radius = ps.BRUSHES["whole"]
        rule = cases["blobs"].rule(centre, 1)
        assert rr.fill(None, *ps.BRUSHES["miss"], ps.SET, 0, rule=lib_rule(rule)) is None
        assert rr.fill(None, centre, radius, ps.SET, 0, 0, (0, 0, 0, 0), rule=lib_rule(rule)) is not None
        assert rr.get_option("blur_scratch_kib") == 0            # no launch, no scratch
        assert_exact(rr.get_volume(), base)
        box, rep = fill(rr, centre, radius, ps.SET, 0, rule)     # 37 x 22 x 45 labels of 4 bytes
        need = 4 * box[1][0] * box[1][1] * box[1][2]
        assert rr.get_option("blur_scratch_kib") == 1024 >= (need + 1023) // 1024   # rounded up to 1 MiB
        once, want_rep = fs.spec_fill(base, centre, radius, ps.SET, 0, rule)
        assert rep == want_rep
        assert_exact(rr.get_volume(), once)
        rr.set_volume(base)
        box, rep = fill(rr, centre, radius, ps.SET, 0, rule)     # the same box: no growth
        assert rr.get_option("blur_scratch_kib") == 1024 and rep == want_rep
        assert_exact(rr.get_volume(), once)
        rr.blur(centre, radius, 2, 1, fs.FULL)                   # a blur within what the fill left
        assert rr.get_option("blur_scratch_kib") == 1024
        assert_exact(rr.get_volume(), bs.spec_blur(once, centre, radius, 2, 1, fs.FULL))


# ---- 8. undo and refusals ----------------------------------------------------------------------
def test_undo(r, cases):
    base = cases["blobs"].vol
    r.set_layout_preference(0)
    r.set_volume(base)
    centre, radius = ps.BRUSHES["straddle"]
    rule = cases["blobs"].rule(centre, 0)
    origin, extent = vr.brush_box(vr.make_brush(centre, radius), DIMS)
    saved = r.get_volume_box(origin, extent)
    box, rep = fill(r, centre, radius, ps.SET, 1, rule, fs.FULL)
    assert box == (origin, extent) and rep[0] > 0
    assert (r.get_volume() != base).any()
    r.update_volume(saved, origin)
    assert_exact(r.get_volume(), base)


def test_refusals(r, cases):
    base = cases["blobs"].vol
    setup(r, 0, base)
    good_b = vr.make_brush((17, 11, 23), (3, 2, 4))
    report = torch.full((vr.FILL_REPORT_BYTES + 8,), 0x5A, dtype=torch.uint8, device="cuda")

    def rule(**kw):
        rl = vr.make_fill_rule((17, 11, 23), 10, 20, (1, 0, 0, 0), 1)
        for k, v in kw.items():
            if k in ("relative", "reserved"):
                setattr(rl, k, v)
            else:
                getattr(rl, k)[:] = v
        return rl

    def refused(b, rl, rep=None, status=1):
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_fill", r._ctx, ctypes.byref(b) if b is not None else None, ctypes.byref(rl) if rl is not None else None,
                      ctypes.c_void_p(rep) if rep else None, None)
        assert e.value.status == status and "vr_fill" in str(e.value)
        torch.cuda.synchronize()
        assert np.array_equal(r.get_volume(), base)
        assert (report == 0x5A).all()

    for rl in (rule(seed=(NX, 11, 23)), rule(seed=(17, -1, 23)), rule(seed=(17, 11, NZ)), rule(relative=2), rule(relative=-1),
               rule(select=(0, 0, 0, 0)), rule(relative=0, lo=(21, 0, 0, 0)), rule(reserved=1)):
        refused(good_b, rl, report.data_ptr())
    for kw in (dict(op=3), dict(falloff=2), dict(radius=(3, 256, 4)), dict(radius=(-1, 2, 4))):
        refused(vr.make_brush(**dict(dict(centre=(17, 11, 23), radius=(3, 2, 4)), **kw)), rule(), report.data_ptr())
    b = vr.make_brush((17, 11, 23), (3, 2, 4))
    b.reserved[1] = 7
    refused(b, rule(), report.data_ptr())
    refused(None, rule())
    refused(good_b, None)
    refused(good_b, rule(), report.data_ptr() + 4)               # a report that is not 8-byte aligned
    assert r.fill(None, (-10, -10, -10), (4, 4, 4), rule=rule()) is None               # a miss is VR_OK
    assert r.fill(None, (17, 11, 23), (3, 2, 4), strength=0, rule=rule()) is not None  # nothing to do is VR_OK too
    assert np.array_equal(r.get_volume(), base)
    check_needs_a_volume(r, lambda rr: rr.fill(None, (17, 11, 23), (3, 2, 4), rule=rule()))
    assert np.array_equal(r.get_volume(), base)
