"""Every arm of the march launchers' dispatch (csrc/vr_dispatch.h) picks a kernel that
computes the right frame: each case is compared bit for bit with the CPU oracle, and
the step counter with the oracle's where it gives one.

The frame is 24 x 16 pixels (3 x 2 wave tiles: ragged workgroups, one entry wave per
XCD, empty XCD lists) and the volume the 16^3 literal (tests/golden).  Its G channel is
uniform as the reference recipe leaves it; "no uniform channel" flips one G texel, and
"channel c uniform" sets channel c of that volume to a constant.  Crossed: the build's
layouts x early-out zero / positive x tap offsets all 0.5 / one not x no / one uniform
channel (each of R, G, B, A on COL48), and for each the launchers vr_render (static,
rings, regions; split 2 / 4 / 8; the LDS slab on COL48), vr_render_rect, vr_render_rects
(two overlapping rectangles), vr_render_pair (both deals) and vr_render_group (four
targets); the procedural medium with and without shadow rays through the sorted,
deferred, tiled, ring, rect and rects launchers.

The image cannot tell a general kernel from the ZO or _u kernel meant; the ordered
kernel names of a run of this file under a kernel trace are compared with the parent
commit's for that (profiles/r10/dispatch).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd import _lib  # noqa: E402
from volumetricrenderer_amd._lib import FMT_RGBA32F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, STEPS = 24, 16, 32
PLANAR, CORNER8, BRICK4832, CORNERH, COL48, COL48Z = 1, 5, 12, 14, 15, 16
DEFAULT_LAYOUTS = {PLANAR: "planar", CORNER8: "corner8", BRICK4832: "brick4832", CORNERH: "cornerh", COL48: "col48"}
EXPERIMENT_LAYOUTS = {2: "brick5", 3: "brick8", 4: "brick16", 6: "brick4", 7: "zpair", 8: "brick448", 9: "brick488",
                      10: "brick4816", 11: "brick41616", 13: "brick4864", COL48Z: "col48z"}
U_LAYOUTS = (COL48, BRICK4832, CORNERH, COL48Z)       # the layouts with _u kernels
FRAME_LAYOUTS = (COL48, BRICK4832, CORNERH)           # ... and with multi-frame kernels
RECT = (3, 2, 17, 11)                                  # across tiles, ragged on every side
COVER = [(0, 0, 16, H), (8, 0, W - 8, H)]              # two overlapping rectangles, union = the frame
SENTINEL = 0xA5


def cases():
    """The build's layouts: an EXPERIMENTS=1 library says so in its build id (vr_get_option "experiments" = 1)."""
    layouts = dict(DEFAULT_LAYOUTS)
    if _lib.load().vr_build_id().decode().endswith("-exp"):
        layouts.update(EXPERIMENT_LAYOUTS)
    out = []
    for layout, name in layouts.items():
        for early in (0.0, 0.05):
            for offs in ("zero", "scroll"):
                for uni in (None, 1) + ((0, 2, 3) if layout == COL48 else ()):
                    cid = f"{name}-early{int(early > 0)}-{offs}-u{'RGBA'[uni] if uni is not None else 'none'}"
                    out.append(pytest.param(layout, early, offs, uni, id=cid))
    return out


@pytest.fixture(scope="module")
def literal():
    v = np.load(os.path.join(ROOT, "tests", "golden", "volume16_literal.npy"))
    assert v.shape == (16, 16, 16, 4) and v.dtype == np.uint8
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module")
def r():
    with vr.Renderer(0) as rr:
        yield rr


def volume(literal, uni):
    """No uniform channel (uni None) or exactly channel uni uniform."""
    v = literal.copy()
    v[3, 5, 7, 1] ^= 0x40   # G is uniform in the literal volume
    if uni is not None:
        v[..., uni] = 102
    for c in range(4):
        assert (v[..., c].min() == v[..., c].max()) == (c == uni)
    return v


def camera(phi, offs):
    osd, gsd = vr.reference_shader_data(W / H, phi, -35.0)
    if offs == "scroll":   # one tap offset not 0.5, inside the clamp-exact range
        gsd.media_scroll[1 * 4 + 1] = 0.01
    return osd, gsd


_refs = {}


def ref_of(oracle, vol, cam, march):
    """Once per (volume, camera, march): the oracle's frame, its steps, the per-pixel step counts."""
    obj, glob = vr.shader_data_arrays(*cam)
    key = (vol.tobytes(), obj.tobytes(), glob.tobytes(), bytes(march))
    if key not in _refs:
        m = oracle.from_params(march)
        img, steps = oracle.render(vol, obj, glob, m, W, H, FMT_RGBA32F)
        n = np.maximum(oracle.step_counts(obj, glob, m, W, H), 0).astype(np.int64)
        img.setflags(write=False)
        _refs[key] = (img, steps, n)
    return _refs[key]


def target(rr):
    out = rr.alloc_target(W, H, FMT_RGBA32F)
    out.view(torch.uint8).fill_(SENTINEL)
    return out


def counter():
    return torch.zeros(1, dtype=torch.int64, device="cuda")


def same(got, want, what):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), what


def masked(ref, rects):
    """A sentinel frame with ref's pixels inside the rectangles."""
    e = np.empty_like(ref)
    e.view(np.uint8).fill(SENTINEL)
    for x, y, w, h in rects:
        e[y:y + h, x:x + w] = ref[y:y + h, x:x + w]
    return e


def reset(rr):
    rr.set_procedural(enabled=0)
    for k, v in (("uniform_skip", 1), ("count", 0), ("split", 1), ("slab", 0), ("schedule", -1), ("pair_deal", 0),
                 ("empty_fill", 1), ("shadow_defer", 1), ("shadow_cache", 0)):
        rr.set_option(k, v)


@pytest.mark.parametrize("layout,early,offs,uni", cases())
def test_grid_launchers(r, oracle, literal, layout, early, offs, uni):
    reset(r)
    vol = volume(literal, uni)
    march = vr.march_defaults(max_steps=STEPS, early_out=early)
    cams = [camera(phi, offs) for phi in (20.0, 21.6, 23.2, 24.8)]
    refs = [ref_of(oracle, vol, c, march) for c in cams]
    ref, steps, n = refs[0]
    assert steps > 0 and ref[..., 0].max() > 0.0   # the volume is on the frame
    try:
        r.set_layout_preference(layout)
        r.set_volume(vol)
        r.set_march(march)
        r.set_shader_data(*cams[0])
        assert r.get_option("uniform_mask") == (0 if uni is None else 1 << uni)
        name = {**DEFAULT_LAYOUTS, **EXPERIMENT_LAYOUTS}[layout]
        variant = r.kernel_variant
        assert name in variant.split("_"), variant
        u_kernel = layout in U_LAYOUTS and uni is not None and early == 0 and offs == "zero"
        assert variant.endswith("_u" + "RGBA"[uni or 0]) == u_kernel, variant

        def whole(what):
            cnt = counter()
            out = r.render(W, H, FMT_RGBA32F, out=target(r), step_counter=cnt)
            torch.cuda.synchronize()
            same(out, ref, what)
            assert int(cnt.item()) == steps, what

        for sched in (0, 4, 5):   # static tiles, rings, regions
            r.set_option("schedule", sched)
            whole(f"schedule {sched}")
        r.set_option("schedule", -1)
        for split in (2, 4, 8):   # lanes per ray (a layout without the split kernels marches one lane per ray)
            r.set_option("split", split)
            whole(f"split {split}")
        r.set_option("split", 1)
        if layout == COL48:
            r.set_option("slab", 1)
            assert "slab" in r.kernel_variant
            whole("slab")
            r.set_option("slab", 0)

        cnt = counter()
        out = r.render_rect(target(r), RECT, FMT_RGBA32F, step_counter=cnt)
        torch.cuda.synchronize()
        same(out, masked(ref, [RECT]), "rect")
        if early == 0:   # the per-pixel counts know no early-out
            x, y, w, h = RECT
            assert int(cnt.item()) == int(n[y:y + h, x:x + w].sum())
        cnt = counter()
        out = r.render_rects(target(r), COVER, FMT_RGBA32F, step_counter=cnt)
        torch.cuda.synchronize()
        same(out, ref, "rects")
        assert int(cnt.item()) == steps   # a pixel both rectangles hold is counted once

        for deal in (0, 1):
            r.set_option("pair_deal", deal)
            cnt, p0 = counter(), r.get_option("pair_launches")
            o0, o1 = r.render_pair(W, H, FMT_RGBA32F, target(r), target(r), cameras=cams[:2], step_counter=cnt)
            torch.cuda.synchronize()
            same(o0, refs[0][0], f"pair deal {deal} frame 0")
            same(o1, refs[1][0], f"pair deal {deal} frame 1")
            assert int(cnt.item()) == refs[0][1] + refs[1][1]
            assert r.get_option("pair_launches") - p0 == (1 if layout in FRAME_LAYOUTS else 0)
        r.set_option("pair_deal", 0)
        cnt, g0 = counter(), r.get_option("group_launches")
        outs = r.render_group(W, H, FMT_RGBA32F, [target(r) for _ in range(4)], cameras=cams, step_counter=cnt)
        torch.cuda.synchronize()
        for i in range(4):
            same(outs[i], refs[i][0], f"group frame {i}")
        assert int(cnt.item()) == sum(x[1] for x in refs)
        assert r.get_option("group_launches") - g0 == (1 if layout in FRAME_LAYOUTS else 0)
    finally:
        reset(r)
        r.set_layout_preference(0)


def test_planar_mirrored_repeat(r, oracle, literal):
    """Tap offsets far outside [0, 1]: only PLANAR's WRAP_MIRROR kernels are exact, whatever the preference."""
    reset(r)
    vol = volume(literal, None)
    march = vr.march_defaults(max_steps=STEPS)
    cam = camera(20.0, "zero")
    for col, vals in enumerate([(0.0, 3.7, -2.2, 1.3), (0.0, -0.6, 5.1, -7.9), (0.0, 1.9, 0.4, -1.1)]):
        for row, v in enumerate(vals):
            cam[1].media_scroll[col * 4 + row] = v
    ref, steps, _ = ref_of(oracle, vol, cam, march)
    try:
        r.set_layout_preference(COL48)
        r.set_volume(vol)
        r.set_march(march)
        r.set_shader_data(*cam)
        assert r.kernel_variant == "grid_planar_mirror"
        for sched in (0, 4, 5):
            r.set_option("schedule", sched)
            cnt = counter()
            same(r.render(W, H, FMT_RGBA32F, out=target(r), step_counter=cnt), ref, f"schedule {sched}")
            assert int(cnt.item()) == steps
        r.set_option("schedule", -1)
        same(r.render_rect(target(r), RECT, FMT_RGBA32F), masked(ref, [RECT]), "rect")
        same(r.render_rects(target(r), COVER, FMT_RGBA32F), ref, "rects")
    finally:
        reset(r)
        r.set_layout_preference(0)


@pytest.mark.parametrize("early", [0.0, 0.01], ids=["early0", "early1"])
@pytest.mark.parametrize("shadow", [0, 5], ids=["cloud", "shadow"])
def test_procedural_launchers(r, oracle, shadow, early):
    reset(r)
    march = vr.march_defaults(max_steps=48, density=40.0, early_out=early)
    cam = camera(20.0, "zero")
    obj, glob = vr.shader_data_arrays(*cam)
    try:
        r.set_shader_data(*cam)
        r.set_march(march)
        r.set_procedural(shadow_steps=shadow)
        p = oracle.procedural_from(r.procedural)
        ref, steps = oracle.render_procedural(p, obj, glob, oracle.from_params(march), W, H, FMT_RGBA32F)
        assert steps > 0 and ref[..., 0].max() > 0.0
        # sorted (with shadow rays: deferred passes, then marched in place), tiles, rings
        for sched, defer, suffix in ((-1, 1, ""), (-1, 0, ""), (0, 1, "_tiles"), (4, 1, "_rings")):
            r.set_option("schedule", sched)
            r.set_option("shadow_defer", defer)
            assert r.kernel_variant == ("procedural_shadow" if shadow else "procedural") + suffix
            cnt = counter()
            out = r.render(W, H, FMT_RGBA32F, out=target(r), step_counter=cnt)
            torch.cuda.synchronize()
            same(out, ref, (sched, defer))
            assert int(cnt.item()) == steps, (sched, defer)
            if sched == -1:
                assert r.get_option("shadow_defer_last") == (1 if shadow and defer else 0)
        r.set_option("schedule", -1)
        r.set_option("shadow_defer", 1)
        same(r.render_rect(target(r), RECT, FMT_RGBA32F), masked(ref, [RECT]), "rect")
        cnt = counter()
        out = r.render_rects(target(r), COVER, FMT_RGBA32F, step_counter=cnt)
        torch.cuda.synchronize()
        same(out, ref, "rects")
        assert int(cnt.item()) == steps
    finally:
        reset(r)
