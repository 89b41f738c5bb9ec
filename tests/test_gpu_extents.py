"""Extent edges: thin, long and limit-size volumes through every march.

Every render call -- render, render_rect of an interior rectangle, render_pair, render_group of four
equal cameras (under the option ladder quad_pairs 1 / quad_pairs 0 / quad_steps 0 / quad_split 0 of
test_gpu_edit_chain) and of four distinct ones (edit_chain.CAMERAS) -- on volumes whose extents sit
where index arithmetic, brick rounding and table sizing can go wrong, for every built layout
(planar, corner8, brick4832, cornerh, col48).  The expected frame is always the CPU oracle's, at
FMT_RGBA8_UNORM and at FMT_RGBA32F, and the comparison is byte for byte.  Counted steps are
compared wherever a call takes a step counter (the QUAD launches count none); vr_query_rect's
per-pixel steps equal oracle.step_counts.  kernel_variant is asserted in every case (no silent
fallback), and for the grouped calls the counters "quad_launches", "quad_split_launches",
"quad_steps_launches", "quad_pairs_launches", "group_launches" and "pair_launches" move as predict()
restates vr_internal.h / vr_render.cpp, from the volume's truly uniform channels.

  1. thin axes: 1x1x1, 1x40x40, 40x1x40, 40x40x1, 2x40x40, 40x40x2, 1x1x64, 3x2x1 -- both trilinear
     corners on one texel, one brick, a slice pair without a partner;
  2. long axes: 4096x2x2, 2x4096x3, 3x2x4096, 600x5x700, cameras along and across the long axis; and the
     LDS-table rule of vr_api.cpp wanted_fast_layout, nx + ny + nz + 3 > 12288 words = 48 KiB: 12281x2x2
     and its transposes run the requested fast layout with the largest tables the library ever builds,
     12282x2x2 and its transposes run the planar kernel;
  3. the CORNERH limit (nx+1)(ny+1)(nz+1) <= 2^24 positions: 4095x63x63 (exactly 2^24) runs cornerh,
     4096x63x63 corner8 under the same preference; the last texel and its seven neighbours carry
     distinct bytes and the camera sits inside a box so large that a tenth of the frame samples them
     (asserted from the oracle: flipping those eight texels changes pixels);
  4. edits on 1x40x40 and 4096x2x2 (col48, brick4832): a paint and a blur centred on the last texel
     with radius 255 along the long axis (more than one 64-lane pass) and an update_volume of a
     sub-box; after each, get_volume is the numpy restatement, render and the four-equal-camera
     render_group are the oracle's frames of it, and update_footprint + render_rect into the frame
     rendered before the edit gives the full re-render.  Every compared frame shows its edit (asserted
     from the oracle); for 4096x2x2 that takes a box stretched along x (LONG_END_BOX).

Volumes are seeded random bytes (default_rng, the seed a function of the extent); a second variant has
one channel constant so that the _u instances run.  Frames are 70 x 37 (quads fall off the right and
the bottom edge), max_steps 16, step_scale 1 and 4, early-out 0 and 0.98, the default unit box (a
stretched volume is sampled anisotropically), targets pre-filled with 0xA5, options as
test_gpu_quad_pairs.setup.  The last test tallies what launched: QUAD_PAIRS, QUAD_STEPS, QUAD_SPLIT
and QUAD_FRAMES, each as a _u and as a general instance, and the planar kernel, on a thin extent and on
a long one.

Not exercised: the last rule of wanted_fast_layout, layout_plane_bytes >= 2^31, needs a volume of
several GB and an oracle pass over it.
"""
import os
import sys
from collections import Counter

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blur_spec as bs  # noqa: E402
import edit_chain as ec  # noqa: E402
import paint_spec as ps  # noqa: E402
from quad_cases import (BRICK4832, COL48, CORNER8, CORNERH, FRAME_LAYOUTS, LADDER, MODES, PLANAR, QUAD_MODES,  # noqa: E402
                        SPLIT_LAYOUTS, counters, predict, refill, set_options as setup)
import quad_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd._lib import FMT_RGBA8_UNORM, FMT_RGBA32F  # noqa: E402

W, H, STEPS = 70, 37, 16
RECT = (9, 5, 43, 21)            # interior, on no tile edge
WHOLE = (0, 0, W, H)
NAMES = {PLANAR: "planar", CORNER8: "corner8", BRICK4832: "brick4832", CORNERH: "cornerh", COL48: "col48"}
BUILT = [PLANAR, CORNER8, BRICK4832, CORNERH, COL48]
FAST = [CORNER8, BRICK4832, CORNERH, COL48]
FORMATS = [(FMT_RGBA8_UNORM, "rgba8"), (FMT_RGBA32F, "rgba32f")]
EARLIES = (0.0, 0.98)
SCALES = (1.0, 4.0)
THIN = [(1, 1, 1), (1, 40, 40), (40, 1, 40), (40, 40, 1), (2, 40, 40), (40, 40, 2), (1, 1, 64), (3, 2, 1)]
LONG = [(4096, 2, 2), (2, 4096, 3), (3, 2, 4096), (600, 5, 700)]
TABLE_WORDS = 12288              # 48 KiB of LDS offset tables
UNDER = [(12281, 2, 2), (2, 12281, 2), (2, 2, 12281)]
OVER = [(12282, 2, 2), (2, 12282, 2), (2, 2, 12282)]
CAMS = [(20.0, -35.0), (0.0, 0.0)]
LONG_CAMS = CAMS + [(90.0, 0.0), (0.0, 89.0)]    # with (0, 0): a view along each of the three axes
# the camera inside a box whose far corner fills the view: the texels at the highest indices
CORNER_BOX = dict(box_min=(-3000.0, -40.0, -40.0), box_max=(0.02, 0.02, 0.02))

TALLY = {"thin": Counter(), "long": Counter()}   # (mode or "planar", "u" or "general") -> launches


def dims_id(d):
    return "x".join(str(v) for v in d)


def volume(dims, uniform):
    """Seeded random bytes (nz, ny, nx, 4); `uniform`: one channel holds one byte -- True: the channel the extent
    picks, (nx + ny + nz) % 4; 0..3: that channel."""
    nx, ny, nz = dims
    v = np.random.default_rng(nx * 1000003 + ny * 1009 + nz).integers(0, 256, size=(nz, ny, nx, 4), dtype=np.uint8)
    if uniform is True:
        v[..., (nx + ny + nz) % 4] = 77
    elif uniform is not False and uniform is not None:
        v[..., int(uniform)] = 77
    return v


# ---- the oracle's frames, once per (volume, camera, march, format) ---------------------------------------------------

def camera(angles):
    return vr.reference_shader_data(W / H, angles[0], angles[1], 0.0)


def march_of(early, scale, box):
    return vr.march_defaults(max_steps=STEPS, step_scale=scale, early_out=early, **(box or {}))


_frames: dict = {}
_steps: dict = {}


def ref(oracle, key, vol, angles, early, scale, fmt, box=None):
    """(frame, counted steps) of the oracle; `key` names the volume's bytes."""
    k = (key, angles, early, scale, fmt, tuple(sorted((box or {}).items())))
    if k not in _frames:
        obj, glob = vr.shader_data_arrays(*camera(angles))
        img, n = oracle.render(vol, obj, glob, oracle.from_params(march_of(early, scale, box)), W, H, fmt)
        img.setflags(write=False)
        _frames[k] = (img, n)
    return _frames[k]


def ref_steps(oracle, angles, scale, box=None):
    """oracle.step_counts: per pixel the steps without early-out, -1 where no ray meets the box."""
    k = (angles, scale, tuple(sorted((box or {}).items())))
    if k not in _steps:
        obj, glob = vr.shader_data_arrays(*camera(angles))
        _steps[k] = oracle.step_counts(obj, glob, oracle.from_params(march_of(0.0, scale, box)), W, H)
    return _steps[k]


def crop(a, rect):
    x, y, w, h = rect
    return a[y:y + h, x:x + w]


# ---- the renderer ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def r():
    with vr.Renderer(0) as rr:
        yield rr


def target(rr, fmt):
    return qc.target(rr, (W, H), fmt)


def counter():
    return torch.zeros(1, dtype=torch.int64, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(got, want, what):
    g = host(got) if isinstance(got, torch.Tensor) else got
    assert g.shape == want.shape and g.dtype == want.dtype, what
    bad = np.argwhere(g.view(np.uint8) != want.view(np.uint8))
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ from the oracle's frame, first (y, x, byte) {bad[:4].tolist()}"


def expect_variant(rr, layout, early, mask, what):
    """The layout's clamp kernel, its _u instance exactly when one channel is uniform and the early-out is off."""
    name = rr.kernel_variant
    assert name.startswith(f"grid_{NAMES[layout]}_clamp"), f"{what}: kernel_variant {name}"
    assert ("_early" in name) == bool(early), f"{what}: kernel_variant {name}"
    u = layout in FRAME_LAYOUTS and not early and mask in (1, 2, 4, 8)     # has_u_kernels, of the built layouts
    tail = "_u" + "RGBA"[mask.bit_length() - 1] if u else ""
    assert ("_u" in name) == u and name.endswith(tail), f"{what}: kernel_variant {name}, uniform mask {mask}"
    return u


def every_call(rr, oracle, key, vol, layout, what, cams=CAMS, box=None, tally=None, earlies=EARLIES, scales=SCALES):
    """Every render call on the installed volume `vol` against the oracle; `layout`: the one that must march."""
    mask = ec.truly_uniform(vol)
    assert rr.get_option("uniform_mask") == mask, f"{what}: uniform_mask"
    four = [camera(a) for a in ec.CAMERAS]
    for early in earlies:
        for scale in scales:
            rr.set_march(march_of(early, scale, box))
            for fmt, fname in FORMATS:
                outs = [target(rr, fmt) for _ in range(4)]
                for angles in cams:
                    at = f"{what}, camera {angles}, early-out {early}, step_scale {scale}, {fname}"
                    cam = camera(angles)
                    rr.set_shader_data(*cam)
                    u = expect_variant(rr, layout, early, mask, at)
                    want, want_n = ref(oracle, key, vol, angles, early, scale, fmt, box)
                    # ---- render
                    cnt = counter()
                    refill(outs[:1])
                    rr.render(W, H, fmt, out=outs[0], step_counter=cnt)
                    same(outs[0], want, f"{at}: render")
                    assert int(cnt.item()) == want_n, f"{at}: render counted {int(cnt.item())} steps, the oracle {want_n}"
                    if tally is not None and layout == PLANAR:
                        tally["planar", "general"] += 1
                    # ---- render_rect: the rectangle's pixels, nothing else
                    cnt = counter()
                    refill(outs[:1])
                    rr.render_rect(outs[0], RECT, fmt, step_counter=cnt)
                    g = host(outs[0])
                    same(np.ascontiguousarray(crop(g, RECT)), np.ascontiguousarray(crop(want, RECT)), f"{at}: render_rect")
                    keep = np.ones((H, W), bool)
                    crop(keep, RECT)[:] = False
                    assert (g.view(np.uint8).reshape(H, W, -1)[keep] == 0xA5).all(), f"{at}: render_rect wrote outside {RECT}"
                    if not early:
                        n = np.maximum(crop(ref_steps(oracle, angles, scale, box), RECT), 0).sum()
                        assert int(cnt.item()) == int(n), f"{at}: render_rect counted {int(cnt.item())} steps, the oracle {int(n)}"
                    # ---- render_pair: this camera and the next of edit_chain.CAMERAS
                    cnt = counter()
                    refill(outs[:2])
                    p0, g0 = rr.get_option("pair_launches"), rr.get_option("group_launches")
                    rr.render_pair(W, H, fmt, outs[0], outs[1], cameras=[cam, four[1]], step_counter=cnt)
                    other, other_n = ref(oracle, key, vol, ec.CAMERAS[1], early, scale, fmt, box)
                    same(outs[0], want, f"{at}: render_pair, frame 0")
                    same(outs[1], other, f"{at}: render_pair, frame 1")
                    assert int(cnt.item()) == want_n + other_n, f"{at}: render_pair counted {int(cnt.item())} steps"
                    assert rr.get_option("pair_launches") - p0 == int(layout in FRAME_LAYOUTS), f"{at}: pair_launches"
                    assert rr.get_option("group_launches") == g0, at
                    # ---- render_group of four equal cameras, under the option ladder
                    for split, steps, pairs in LADDER:
                        for opt, v in (("quad_split", split), ("quad_steps", steps), ("quad_pairs", pairs)):
                            rr.set_option(opt, v)
                        refill(outs)
                        c0, g0 = counters(rr), rr.get_option("group_launches")
                        rr.render_group(W, H, fmt, outs, cameras=[cam] * 4)
                        torch.cuda.synchronize()
                        moved = tuple(b - a for a, b in zip(c0, counters(rr)))
                        opts = f"quad_split {split}, quad_steps {steps}, quad_pairs {pairs}"
                        assert moved == predict(layout, early, mask, split, steps, pairs), \
                            f"{at}, {opts}: (QUAD, split, step-round, paired) launches {moved}"
                        assert rr.get_option("group_launches") - g0 == int(layout in FRAME_LAYOUTS), f"{at}: group_launches"
                        for i in range(4):
                            same(outs[i], want, f"{at}: render_group of one camera, {opts}, frame {i}")
                        if tally is not None:
                            tally[MODES[moved], "u" if u else "general"] += 1
                    for opt in ("quad_split", "quad_steps", "quad_pairs"):
                        rr.set_option(opt, 1)
                # ---- render_group of four distinct cameras: never a QUAD launch
                at = f"{what}, early-out {early}, step_scale {scale}, {fname}"
                cnt = counter()
                refill(outs)
                c0, g0 = counters(rr), rr.get_option("group_launches")
                rr.render_group(W, H, fmt, outs, cameras=four, step_counter=cnt)
                total = 0
                for i in range(4):
                    want, n = ref(oracle, key, vol, ec.CAMERAS[i], early, scale, fmt, box)
                    same(outs[i], want, f"{at}: render_group of four cameras, frame {i}")
                    total += n
                assert int(cnt.item()) == total, f"{at}: render_group counted {int(cnt.item())} steps, the oracle {total}"
                assert counters(rr) == c0, f"{at}: a QUAD launch for frames of different cameras"
                assert rr.get_option("group_launches") - g0 == int(layout in FRAME_LAYOUTS), f"{at}: group_launches"
    # ---- vr_query_rect's steps, per pixel
    for scale in scales:
        rr.set_march(march_of(0.0, scale, box))
        for angles in cams:
            rr.set_shader_data(*camera(angles))
            n = ref_steps(oracle, angles, scale, box)
            rec = vr.ray_records(rr.query_rect(WHOLE, W, H))
            assert np.array_equal(rec["steps"], n), f"{what}, camera {angles}, step_scale {scale}: query_rect steps"
            part = vr.ray_records(rr.query_rect(RECT, W, H))
            assert np.array_equal(part["steps"], crop(n, RECT)), f"{what}, camera {angles}, step_scale {scale}: query_rect of {RECT}"


def both_variants(rr, oracle, dims, pref, layout, cams=CAMS, tally=None):
    setup(rr, pref)
    for uniform in (False, True):
        vol = volume(dims, uniform)
        rr.set_volume(vol)
        what = f"{dims_id(dims)}{' (one channel uniform)' if uniform else ''}, preference {NAMES[pref]}"
        every_call(rr, oracle, (dims, uniform), vol, layout, what, cams=cams, tally=tally)


# ---- 1. thin axes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pref", BUILT, ids=[NAMES[p] for p in BUILT])
@pytest.mark.parametrize("dims", THIN, ids=dims_id)
def test_thin_axes(r, oracle, dims, pref):
    both_variants(r, oracle, dims, pref, pref, tally=TALLY["thin"])


# ---- 2. long axes and the LDS-table rule -----------------------------------------------------------------------------

@pytest.mark.parametrize("pref", BUILT, ids=[NAMES[p] for p in BUILT])
@pytest.mark.parametrize("dims", LONG, ids=dims_id)
def test_long_axes(r, oracle, dims, pref):
    assert sum(dims) + 3 < TABLE_WORDS
    both_variants(r, oracle, dims, pref, pref, cams=LONG_CAMS, tally=TALLY["long"])


@pytest.mark.parametrize("pref", FAST, ids=[NAMES[p] for p in FAST])
@pytest.mark.parametrize("dims", UNDER, ids=dims_id)
def test_largest_offset_tables(r, oracle, dims, pref):
    """nx + ny + nz + 3 = 12288 words: the requested layout marches, with 48 KiB of tables (none for cornerh)."""
    assert sum(dims) + 3 == TABLE_WORDS
    both_variants(r, oracle, dims, pref, pref, cams=LONG_CAMS, tally=TALLY["long"])


@pytest.mark.parametrize("pref", FAST, ids=[NAMES[p] for p in FAST])
@pytest.mark.parametrize("dims", OVER, ids=dims_id)
def test_one_word_past_the_tables_is_planar(r, oracle, dims, pref):
    assert sum(dims) + 3 == TABLE_WORDS + 1
    both_variants(r, oracle, dims, pref, PLANAR, cams=LONG_CAMS, tally=TALLY["long"])


# ---- 3. the CORNERH limit --------------------------------------------------------------------------------------------

AT_LIMIT, PAST_LIMIT = (4095, 63, 63), (4096, 63, 63)
CORNER_BYTES = np.array([[(13 * i + 7 * c + 5) % 256 for c in range(4)] for i in range(8)], np.uint8).reshape(2, 2, 2, 4)


def limit_volume(dims, uniform):
    v = volume(dims, uniform)
    q = (sum(dims)) % 4
    v[-2:, -2:, -2:, :] = CORNER_BYTES          # the last texel and its seven neighbours
    if uniform:
        v[..., q] = 77
    return v, q


@pytest.fixture(scope="module", params=[(d, u) for d in (AT_LIMIT, PAST_LIMIT) for u in (False, True)],
                ids=lambda p: dims_id(p[0]) + ("-uniform" if p[1] else ""))
def at_the_limit(request):
    """One install per volume and module: a Renderer of its own, closed (and its GiB of cornerh planes freed) after."""
    dims, uniform = request.param
    vol, q = limit_volume(dims, uniform)
    with vr.Renderer(0) as rr:
        setup(rr, CORNERH)
        rr.set_volume(vol)
        yield rr, dims, uniform, vol, q


def test_cornerh_limit(at_the_limit, oracle):
    rr, dims, uniform, vol, q = at_the_limit
    positions = (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1)
    layout = CORNERH if positions <= 2**24 else CORNER8
    assert (positions == 2**24) == (dims == AT_LIMIT) and (positions > 2**24) == (dims == PAST_LIMIT)
    what = f"{dims_id(dims)}{' (one channel uniform)' if uniform else ''}, preference cornerh"
    # the frames do sample the eight texels of the highest indices: the oracle's change when they do
    flipped = vol.copy()
    flipped[-2:, -2:, -2:, [c for c in range(4) if not (uniform and c == q)]] ^= 0xFF
    for angles in CAMS:
        for scale in SCALES:
            a, _ = ref(oracle, (dims, uniform), vol, angles, 0.0, scale, FMT_RGBA8_UNORM, CORNER_BOX)
            b, _ = ref(oracle, (dims, uniform, "flipped"), flipped, angles, 0.0, scale, FMT_RGBA8_UNORM, CORNER_BOX)
            changed = int((a != b).any(axis=2).sum())
            print(f"{what}, camera {angles}, step_scale {scale}: {changed} pixels sample the last eight texels")
            assert changed >= W * H // 20, f"{what}: only {changed} pixels sample the last eight texels"
    del flipped
    every_call(rr, oracle, (dims, uniform), vol, layout, what + ", the far corner", box=CORNER_BOX)
    every_call(rr, oracle, (dims, uniform), vol, layout, what + ", the unit box", scales=(4.0,))


# ---- 4. edits on a thin and on a long extent -------------------------------------------------------------------------

# In the unit box no pixel of these frames samples the last sixteenth of 4096x2x2's long axis (the oracle's frames
# before and after the paint are equal), so that extent's box is stretched along x until the brush fills its near end.
LONG_END_BOX = dict(box_min=(-31.0, -1.0, -1.0), box_max=(1.0, 1.0, 1.0))
EDIT_EXTENTS = {(1, 40, 40): ("thin", None), (4096, 2, 2): ("long", LONG_END_BOX)}


def edits_of(dims, q):
    """[(name, run(renderer) -> returned box, apply(volume) -> volume, (origin, extent))]: a paint and a blur centred on
    the last texel, radius 255 along the longest axis, strength 0 on channel q; an update_volume of a sub-box."""
    last = tuple(n - 1 for n in dims)
    long_axis = int(np.argmax(dims))
    radius = tuple(255 if ax == long_axis else min(1, dims[ax] - 1) if ax == 0 else min(6, dims[ax] - 1) for ax in range(3))
    strength = tuple(0 if c == q else s for c, s in enumerate((255, 200, 230, 255)))
    box = ps.spec_box(last, radius, dims)
    assert box is not None and box[1][long_axis] == min(256, dims[long_axis])
    sub_o = tuple(max(0, n - 1 - min(n - 1, 70)) for n in dims)
    sub_e = tuple(min(n - o, 61) for n, o in zip(dims, sub_o))
    patch = np.random.default_rng(sum(dims)).integers(0, 256, size=(sub_e[2], sub_e[1], sub_e[0], 4), dtype=np.uint8)

    def updated(v):
        out = v.copy()
        out[sub_o[2]:sub_o[2] + sub_e[2], sub_o[1]:sub_o[1] + sub_e[1], sub_o[0]:sub_o[0] + sub_e[0]] = patch
        return out
    return [
        ("paint", lambda rr: rr.paint(last, radius, ps.SET, 1, ps.VALUE, strength),
         lambda v: ps.spec_apply(v, last, radius, ps.SET, 1, ps.VALUE, strength), box),
        ("blur", lambda rr: rr.blur(last, radius, 2, 1, strength),
         lambda v: bs.spec_blur(v, last, radius, 2, 1, strength), box),
        ("update_volume", lambda rr: rr.update_volume(patch, sub_o) or (sub_o, sub_e), updated, (sub_o, sub_e)),
    ]


@pytest.mark.parametrize("uniform", [False, True], ids=["general", "uniform"])
@pytest.mark.parametrize("pref", SPLIT_LAYOUTS, ids=[NAMES[p] for p in SPLIT_LAYOUTS])
@pytest.mark.parametrize("dims", list(EDIT_EXTENTS), ids=dims_id)
def test_edits(r, oracle, dims, pref, uniform):
    # the constant channel, which the brushes leave alone: never R, the one tap that samples the whole box
    # (tap_scale 1; G, B and A stop at 0.8, 0.75 and 0.7 of it and never reach an axis's last sixteenth)
    q = 1 + sum(dims) % 3
    angles, fmt = CAMS[0], FMT_RGBA8_UNORM
    kind, box3 = EDIT_EXTENTS[dims]
    vols = [volume(dims, q if uniform else False)]
    edits = edits_of(dims, q)
    for _, _, apply, _ in edits:
        vols.append(np.ascontiguousarray(apply(vols[-1])))
    setup(r, pref)
    r.set_volume(vols[0])
    cam = camera(angles)
    seen = 0
    mask = 15
    for k, vol in enumerate(vols):
        name = edits[k - 1][0] if k else "install"
        what = f"{dims_id(dims)}, {NAMES[pref]}, step {k} {name}"
        mask &= ec.truly_uniform(vol)         # the mask can only be lost (vr.h vr_update_volume)
        earlier = {}
        if k:
            _, run, _, box = edits[k - 1]
            # frames of the volume before the edit, one per march, to be patched by render_rect
            for early in EARLIES:
                for scale in SCALES:
                    r.set_march(march_of(early, scale, box3))
                    r.set_shader_data(*cam)
                    earlier[early, scale] = r.render(W, H, fmt, out=target(r, fmt))
                    same(earlier[early, scale], ref(oracle, (dims, uniform, k - 1), vols[k - 1], angles, early, scale, fmt, box3)[0],
                         f"{what}: the frame before the edit")
            assert run(r) == box, f"{what}: the returned box"
        got = r.get_volume()
        bad = np.argwhere(got != vol)
        assert bad.size == 0, f"{what}: get_volume differs at {len(bad)} bytes, first (z, y, x, c) {bad[:4].tolist()}"
        assert r.get_option("uniform_mask") == mask, f"{what}: uniform_mask {r.get_option('uniform_mask')}, expected {mask}"
        for early in EARLIES:
            for scale in SCALES:
                at = f"{what}, early-out {early}, step_scale {scale}"
                r.set_march(march_of(early, scale, box3))
                r.set_shader_data(*cam)
                u = expect_variant(r, pref, early, mask, at)
                want = ref(oracle, (dims, uniform, k), vol, angles, early, scale, fmt, box3)[0]
                if k:
                    seen += int((want != ref(oracle, (dims, uniform, k - 1), vols[k - 1], angles, early, scale, fmt, box3)[0]).any())
                    # update_footprint of the edited box, render_rect into the earlier frame: the full re-render
                    rect = r.update_footprint(*edits[k - 1][3], W, H)
                    assert rect[2] > 0 and rect[3] > 0, f"{at}: the edited box has no footprint"
                    r.render_rect(earlier[early, scale], rect, fmt)
                    same(earlier[early, scale], want, f"{at}: update_footprint {rect} + render_rect into the earlier frame")
                outs = [target(r, fmt) for _ in range(4)]
                r.render(W, H, fmt, out=outs[0])
                same(outs[0], want, f"{at}: render")
                refill(outs[:1])
                c0 = counters(r)
                r.render_group(W, H, fmt, outs, cameras=[cam] * 4)
                torch.cuda.synchronize()
                moved = tuple(b - a for a, b in zip(c0, counters(r)))
                assert moved == predict(pref, early, mask, 1, 1, 1), f"{at}: (QUAD, split, step-round, paired) launches {moved}"
                for i in range(4):
                    same(outs[i], want, f"{at}: render_group of one camera, frame {i}")
                TALLY[kind][MODES[moved], "u" if u else "general"] += 1
    assert seen == len(edits) * len(EARLIES) * len(SCALES), f"{dims_id(dims)}: only {seen} of the compared frames show their edit"


# ---- what launched ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["thin", "long"])
def test_every_mode_ran(r, oracle, kind):
    """QUAD_PAIRS, QUAD_STEPS, QUAD_SPLIT and QUAD_FRAMES as a _u and as a general instance, the general instance's
    predicted 0 (COL48 / BRICK4832 without early-out), and the planar kernel, each counted at least once on an extent
    of this kind by the tests above.  Run on its own (nothing tallied yet) it first walks one extent itself."""
    tally = TALLY[kind]
    if not tally:
        dims = THIN[1] if kind == "thin" else LONG[0]
        for pref in (COL48, PLANAR):
            both_variants(r, oracle, dims, pref, pref, tally=tally)
    print(f"{kind} extents: counted launches {dict(tally)}")
    for mode in QUAD_MODES:
        for inst in ("u", "general"):
            assert tally[mode, inst] > 0, f"{kind} extents: no {mode} launch of the {inst} instance; {dict(tally)}"
    assert tally["QUAD_NONE", "general"] > 0 and tally["planar", "general"] > 0, dict(tally)
