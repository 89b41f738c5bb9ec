"""vr_render_rect (the scissored render) and the edit loop `update box ->
re-render its footprint` on the GPU, against the CPU oracle.  Every comparison
is exact: pixels bit for bit, whole buffers byte for byte, counters equal.

Scissor parity renders a 67 x 45 frame (neither side a multiple of the 8 x 8
wave tile) into a sentinel-filled buffer with a padded row pitch and guard
rows, and compares the WHOLE buffer: the oracle's frame inside the rectangle,
the sentinel everywhere else.  The edit loop uses the boxes and cameras of
tests/test_gpu_update.py (37 x 22 x 45 random bytes, 64 x 64, 32 steps).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd import _lib  # noqa: E402
from volumetricrenderer_amd._lib import (FMT_R8_SRGB, FMT_R8_UNORM, FMT_R32F, FMT_RGBA8_SRGB,  # noqa: E402
                                         FMT_RGBA8_UNORM, FMT_RGBA32F, VRError)

NX, NY, NZ = 37, 22, 45
STEPS = 32
LAYOUTS = [(1, "planar"), (5, "corner8"), (12, "brick4832"), (14, "cornerh"), (15, "col48")]
LAYOUT_IDS = [n for _, n in LAYOUTS]
UNIFORM_VARIANTS = [(p, n) for p, n in LAYOUTS if p in (12, 14, 15)]   # the layouts with _uX kernels

FW, FH = 67, 45
RECTS = {
    "first_pixel": (0, 0, 1, 1),
    "last_pixel": (FW - 1, FH - 1, 1, 1),
    "full_row": (0, 17, FW, 1),
    "full_column": (29, 0, 1, FH),
    "unaligned_in_tile_pair": (3, 5, 9, 7),
    "straddles_tiles": (5, 6, 40, 30),
    "whole_frame": (0, 0, FW, FH),
    "overhanging_corner": (60, 40, 7, 5),
    "empty": (10, 10, 0, 5),
}
ALL_FORMATS = (FMT_RGBA32F, FMT_RGBA8_UNORM, FMT_RGBA8_SRGB, FMT_R8_UNORM, FMT_R8_SRGB, FMT_R32F)
GUARD, PAD = 3, 5      # guard rows above and below, padding pixels at the end of each row
COUNT0 = 1000          # the counter's non-zero start

# the edit loop: name -> (origin, extent, camera (phi, theta)), tests/test_gpu_update.py BOXES
BOXES = {
    "interior_texel": ((17, 11, 23), (1, 1, 1), (0.0, 0.0)),
    "corner_000": ((0, 0, 0), (1, 1, 1), (180.0, 60.0)),
    "corner_x00": ((NX - 1, 0, 0), (1, 1, 1), (60.0, -60.0)),
    "corner_0y0": ((0, NY - 1, 0), (1, 1, 1), (240.0, 60.0)),
    "corner_xy0": ((NX - 1, NY - 1, 0), (1, 1, 1), (30.0, -60.0)),
    "corner_00z": ((0, 0, NZ - 1), (1, 1, 1), (180.0, 0.0)),
    "corner_x0z": ((NX - 1, 0, NZ - 1), (1, 1, 1), (90.0, 0.0)),
    "corner_0yz": ((0, NY - 1, NZ - 1), (1, 1, 1), (270.0, 0.0)),
    "corner_xyz": ((NX - 1, NY - 1, NZ - 1), (1, 1, 1), (0.0, 0.0)),
    "straddle_5x9x34": ((2, 6, 30), (34, 9, 5), (0.0, 0.0)),
    "z_slab": ((0, 0, NZ - 1), (NX, NY, 1), (0.0, 0.0)),
    "x_row": ((0, 0, 0), (NX, 1, 1), (180.0, 60.0)),
}
EW = EH = 64


@pytest.fixture(scope="module")
def base():
    return np.random.default_rng(20240607).integers(0, 256, size=(NZ, NY, NX, 4), dtype=np.uint8)


@pytest.fixture(scope="module")
def r():
    with vr.Renderer(0) as rr:
        yield rr


def setup(rr, pref, vol, osd, gsd, march=None):
    rr.set_procedural(enabled=0)
    rr.set_option("uniform_skip", 1)
    rr.set_option("count", 0)
    rr.set_layout_preference(pref)
    rr.set_volume(vol)
    rr.set_shader_data(osd, gsd)
    rr.set_march(march if march is not None else vr.march_defaults(max_steps=STEPS))


_refs = {}


def oracle_refs(oracle, vol, osd, gsd, march, w, h):
    """Once per (volume, camera, march, size): the oracle's RGBA32F and RGBA8
    frames, its executed steps and the per-pixel step counts."""
    obj, glob = vr.shader_data_arrays(osd, gsd)
    m = oracle.from_params(march)
    key = (hash(vol.tobytes()), obj.tobytes(), glob.tobytes(), bytes(march), w, h)
    if key not in _refs:
        f32, steps = oracle.render(vol, obj, glob, m, w, h, FMT_RGBA32F)
        u8, _ = oracle.render(vol, obj, glob, m, w, h, FMT_RGBA8_UNORM)
        n = np.maximum(oracle.step_counts(obj, glob, m, w, h), 0).astype(np.int64)
        _refs[key] = (f32, u8, steps, n)
    return _refs[key]


def sentinel_buffer(fmt, w=FW, h=FH):
    """(whole buffer, the frame's view of it): guard rows around the frame and
    PAD pixels after each row, every byte the sentinel 0xA5."""
    dt = torch.float32 if fmt in _lib.FLOAT_FORMATS else torch.uint8
    shape = (h + 2 * GUARD, w + PAD) + ((4,) if _lib.CHANNELS[fmt] == 4 else ())
    buf = torch.empty(shape, dtype=dt, device="cuda")
    buf.view(torch.uint8).fill_(0xA5)
    return buf, buf[GUARD:GUARD + h, :w]


def expect_buffer(buf_shape, dtype, ref, rect):
    """The sentinel buffer with `ref`'s pixels inside the rectangle."""
    e = np.empty(buf_shape, dtype)
    e.view(np.uint8).fill(0xA5)
    x, y, w, h = rect
    e[GUARD + y:GUARD + y + h, x:x + w] = ref[y:y + h, x:x + w]
    return e


def assert_bytes_equal(got, want, what):
    g, w = got.view(np.uint8).reshape(got.shape[0], -1), want.view(np.uint8).reshape(want.shape[0], -1)
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} differing bytes, first (row, byte) {bad[:6].tolist()}"


def rect_sum(n, rect):
    x, y, w, h = rect
    return int(n[y:y + h, x:x + w].sum())


def check_rects(rr, refs_of_fmt, n, formats, rects, what):
    """render_rect of every (format, rectangle) into a fresh sentinel buffer:
    the whole buffer and the counter afterwards."""
    for fmt in formats:
        ref = refs_of_fmt(fmt)
        for rname, rect in rects.items():
            buf, view = sentinel_buffer(fmt, ref.shape[1], ref.shape[0])
            cnt = torch.full((1,), COUNT0, dtype=torch.int64, device="cuda")
            rr.render_rect(view, rect, fmt, step_counter=cnt)
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert_bytes_equal(got, expect_buffer(got.shape, got.dtype, ref, rect), f"{what} fmt {fmt} {rname} {rect}")
            if n is not None:
                assert int(cnt.item()) == COUNT0 + rect_sum(n, rect), (what, fmt, rname)


# ---- scissor parity -------------------------------------------------------------
@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_scissor_parity(r, oracle, base, pref, name):
    osd, gsd = vr.reference_shader_data(FW / FH)
    march = vr.march_defaults(max_steps=STEPS)
    setup(r, pref, base, osd, gsd, march)
    assert r.kernel_variant.startswith(f"grid_{name}_clamp"), r.kernel_variant
    f32, u8, steps, n = oracle_refs(oracle, base, osd, gsd, march, FW, FH)
    assert steps == n.sum() > 0
    own = {}   # the sRGB formats: vr_render's own frame (the oracle is within 1 LSB there)
    for fmt in (FMT_RGBA8_SRGB, FMT_R8_SRGB):
        own[fmt] = r.render(FW, FH, fmt).cpu().numpy()
    assert np.abs(own[FMT_RGBA8_SRGB][..., 0].astype(int) - own[FMT_R8_SRGB].astype(int)).max() == 0
    refs = {FMT_RGBA32F: f32, FMT_RGBA8_UNORM: u8, FMT_R32F: f32[..., 0], FMT_R8_UNORM: u8[..., 0], **own}
    # vr_render itself agrees with the oracle here, so "what vr_render writes there" is the oracle's frame
    assert np.array_equal(r.render(FW, FH, FMT_RGBA32F).cpu().numpy(), f32)
    check_rects(r, refs.__getitem__, n, ALL_FORMATS, RECTS, name)


def _mirror_case():
    osd, gsd = vr.reference_shader_data(FW / FH)
    gsd.media_scroll[0 * 4 + 1] = 1.5    # tap 1: u = 0.8 P + 0.3 along x, past 1: mirrored repeat
    gsd.media_scroll[1 * 4 + 2] = -1.0   # tap 2: u from -0.25 along y
    return osd, gsd, vr.march_defaults(max_steps=STEPS), "grid_planar_mirror"


def _early_case():
    osd, gsd = vr.reference_shader_data(FW / FH)
    return osd, gsd, vr.march_defaults(max_steps=STEPS, density=16.0, early_out=0.5), None


def _rotated_case():
    osd, gsd = vr.reference_shader_data(FW / FH, 40.0, 25.0)
    return osd, gsd, vr.march_defaults(max_steps=STEPS), None


def _cam_off_eye_case():
    osd, gsd = vr.reference_shader_data(FW / FH)
    gsd.camera_position[0] += 0.5        # cam_mode 1: the march starts off the projection centre
    gsd.camera_position[2] -= 0.25
    return osd, gsd, vr.march_defaults(max_steps=STEPS), None


VARIANT_CASES = {"mirrored_repeat": _mirror_case, "early_out": _early_case, "rotated_camera": _rotated_case,
                 "camera_off_eye": _cam_off_eye_case}
VARIANT_RECTS = {k: RECTS[k] for k in ("unaligned_in_tile_pair", "straddles_tiles", "whole_frame",
                                       "overhanging_corner")}


@pytest.mark.parametrize("case", list(VARIANT_CASES))
@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_scissor_variants(r, oracle, base, pref, name, case):
    osd, gsd, march, variant = VARIANT_CASES[case]()
    setup(r, pref, base, osd, gsd, march)
    if variant:
        assert r.kernel_variant == variant   # every layout falls back to the planar mirrored march
    elif case == "early_out":
        assert r.kernel_variant.endswith("_early")
    f32, _, steps, n = oracle_refs(oracle, base, osd, gsd, march, FW, FH)
    if case == "early_out":
        assert 0 < steps < n.sum(), "early_out stops no ray: the case shows nothing"
        check_rects(r, lambda fmt: f32, None, (FMT_RGBA32F,), VARIANT_RECTS, case)
        cnt = torch.full((1,), COUNT0, dtype=torch.int64, device="cuda")
        r.render_rect(sentinel_buffer(FMT_RGBA32F)[1], RECTS["whole_frame"], FMT_RGBA32F, step_counter=cnt)
        assert int(cnt.item()) == COUNT0 + steps
    else:
        check_rects(r, lambda fmt: f32, n, (FMT_RGBA32F,), VARIANT_RECTS, case)


# ---- procedural medium ----------------------------------------------------------
PW, PH, PSTEPS = 48, 40, 16
PROC_RECTS = {"unaligned": (3, 5, 9, 7), "straddles_tiles": (5, 6, 30, 20), "whole_frame": (0, 0, PW, PH)}


@pytest.mark.parametrize("shadow", [0, 3])
def test_procedural_rect(r, oracle, shadow):
    osd, gsd = vr.reference_shader_data(PW / PH, 20.0, 15.0)
    march = vr.march_defaults(max_steps=PSTEPS)
    r.set_shader_data(osd, gsd)
    r.set_march(march)
    r.set_procedural(shadow_steps=shadow)
    try:
        obj, glob = vr.shader_data_arrays(osd, gsd)
        m = oracle.from_params(march)
        ref, steps, evals = oracle.render_procedural(oracle.procedural_from(r.procedural), obj, glob, m, PW, PH,
                                                     FMT_RGBA32F, with_evals=True)
        n = np.maximum(oracle.step_counts(obj, glob, m, PW, PH), 0).astype(np.int64)
        assert steps == n.sum() > 0 and ref[..., 0].max() > 0.0
        assert (evals > steps) == (shadow > 0)
        check_rects(r, lambda fmt: ref, n, (FMT_RGBA32F,), PROC_RECTS, f"procedural shadow {shadow}")
        r.set_option("count", 1)   # density evaluations: ray-steps plus shadow samples
        cnt = torch.full((1,), COUNT0, dtype=torch.int64, device="cuda")
        r.render_rect(sentinel_buffer(FMT_RGBA32F, PW, PH)[1], PROC_RECTS["whole_frame"], FMT_RGBA32F,
                      step_counter=cnt)
        assert int(cnt.item()) == COUNT0 + evals
        # two rectangles that tile the frame count what the frame counts
        cnt.fill_(0)
        for rect in ((0, 0, 21, PH), (21, 0, PW - 21, PH)):
            r.render_rect(sentinel_buffer(FMT_RGBA32F, PW, PH)[1], rect, FMT_RGBA32F, step_counter=cnt)
        assert int(cnt.item()) == evals
    finally:
        r.set_option("count", 0)
        r.set_procedural(enabled=0)


# ---- the edit loop --------------------------------------------------------------
def inverted_box(vol, origin, extent):
    (x0, y0, z0), (bx, by, bz) = origin, extent
    return 255 - vol[z0:z0 + bz, y0:y0 + by, x0:x0 + bx]


def patch_into(vol, box, origin):
    x0, y0, z0 = origin
    bz, by, bx, _ = box.shape
    out = vol.copy()
    out[z0:z0 + bz, y0:y0 + by, x0:x0 + bx] = box
    return out


@pytest.mark.parametrize("boxname", list(BOXES))
@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_edit_loop(r, oracle, base, pref, name, boxname):
    origin, extent, angles = BOXES[boxname]
    osd, gsd = vr.reference_shader_data(1.0, *angles)
    march = vr.march_defaults(max_steps=STEPS)
    setup(r, pref, base, osd, gsd, march)
    assert r.kernel_variant.startswith(f"grid_{name}_clamp"), r.kernel_variant
    frame = r.render(EW, EH, FMT_RGBA32F)
    box = inverted_box(base, origin, extent)
    r.update_volume(box, origin)
    fp = r.update_footprint(origin, extent, EW, EH)
    assert 0 < fp[2] and 0 < fp[3]
    r.render_rect(frame, fp, FMT_RGBA32F)
    torch.cuda.synchronize()
    want, _, _, _ = oracle_refs(oracle, patch_into(base, box, origin), osd, gsd, march, EW, EH)
    before, _, _, _ = oracle_refs(oracle, base, osd, gsd, march, EW, EH)
    assert (want != before).any(), "the edit changes nothing: the case shows nothing"
    got = frame.cpu().numpy()
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, f"footprint {fp}: {len(bad)} stale or wrong pixels, first (y, x) {bad[:6].tolist()}"


@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_edit_loop_queued_device_updates(r, oracle, base, pref, name):
    """Three device-side edits and their footprint renders queued back to back
    on one stream, no host wait in between."""
    osd, gsd = vr.reference_shader_data(1.0)
    march = vr.march_defaults(max_steps=STEPS)
    setup(r, pref, base, osd, gsd, march)
    rng = np.random.default_rng(31)
    edits = [((2, 6, 30), (34, 9, 5)), ((17, 11, 23), (1, 1, 1)), ((20, 3, 10), (9, 12, 20))]
    boxes = [rng.integers(0, 256, size=(bz, by, bx, 4), dtype=np.uint8) for _, (bx, by, bz) in edits]
    dev = [torch.from_numpy(b).cuda() for b in boxes]   # uploaded before the loop: nothing below waits
    frame = r.alloc_target(EW, EH, FMT_RGBA32F)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    patched = base
    r.render(EW, EH, FMT_RGBA32F, out=frame, stream=s)
    for (origin, extent), box, d in zip(edits, boxes, dev):
        r.update_volume(d, origin, stream=s)
        r.render_rect(frame, r.update_footprint(origin, extent, EW, EH), FMT_RGBA32F, stream=s)
        patched = patch_into(patched, box, origin)
    s.synchronize()
    want, _, _, _ = oracle_refs(oracle, patched, osd, gsd, march, EW, EH)
    assert np.array_equal(frame.cpu().numpy(), want)


@pytest.mark.parametrize("keeps_uniform", [False, True], ids=["breaks_G", "keeps_G"])
@pytest.mark.parametrize("pref,name", UNIFORM_VARIANTS, ids=[n for _, n in UNIFORM_VARIANTS])
def test_edit_loop_with_a_uniform_channel(r, oracle, base, pref, name, keeps_uniform):
    """G uniform at the edit (the recipe's G): the rectangle march loads every
    channel and leaves the pending read-back to the next vr_render."""
    vol = base.copy()
    vol[..., 1] = 137
    osd, gsd = vr.reference_shader_data(1.0)
    march = vr.march_defaults(max_steps=STEPS)
    setup(r, pref, vol, osd, gsd, march)
    assert r.kernel_variant.endswith("_uG"), r.kernel_variant
    frame = r.render(EW, EH, FMT_RGBA32F)
    origin, extent = (16, 10, 22), (3, 3, 3)
    box = inverted_box(vol, origin, extent)
    box[..., 1] = 137 if keeps_uniform else 138
    r.update_volume(box, origin)
    r.render_rect(frame, r.update_footprint(origin, extent, EW, EH), FMT_RGBA32F)
    torch.cuda.synchronize()
    want, _, _, _ = oracle_refs(oracle, patch_into(vol, box, origin), osd, gsd, march, EW, EH)
    assert np.array_equal(frame.cpu().numpy(), want)
    # the next vr_render resolves the read-back as it does without the rectangle render
    again = r.render(EW, EH, FMT_RGBA32F).cpu().numpy()
    assert np.array_equal(again, want)
    assert bool(r.get_option("uniform_mask") & 2) == keeps_uniform
    assert r.kernel_variant.endswith("_uG") == keeps_uniform


# ---- no side effects --------------------------------------------------------------
def test_rect_leaves_the_launch_cache_alone(r, oracle, base):
    osd, gsd = vr.reference_shader_data(1.0)
    setup(r, 0, base, osd, gsd)
    out = r.alloc_target(EW, EH, FMT_RGBA32F)
    other = r.alloc_target(EW, EH, FMT_RGBA32F)
    r.render(EW, EH, FMT_RGBA32F, out=out)
    h0 = r.get_option("launch_cache_hits")
    r.render(EW, EH, FMT_RGBA32F, out=out)
    h1 = r.get_option("launch_cache_hits")
    assert h1 == h0 + 1   # the baseline: a repeated render is a hit
    first = out.cpu().numpy()
    r.render_rect(other, (5, 6, 40, 30), FMT_RGBA32F)
    r.render_rect(out, (5, 6, 40, 30), FMT_RGBA32F)
    assert r.get_option("launch_cache_hits") == h1
    r.render(EW, EH, FMT_RGBA32F, out=out)
    assert r.get_option("launch_cache_hits") == h1 + 1
    assert np.array_equal(out.cpu().numpy(), first)


def test_rect_between_sorted_procedural_renders(r, oracle):
    osd, gsd = vr.reference_shader_data(PW / PH, 20.0, 15.0)
    march = vr.march_defaults(max_steps=PSTEPS)
    r.set_shader_data(osd, gsd)
    r.set_march(march)
    r.set_procedural(shadow_steps=3)
    try:
        assert r.kernel_variant == "procedural_shadow"   # the cost-sorted schedule
        obj, glob = vr.shader_data_arrays(osd, gsd)
        ref, _ = oracle.render_procedural(oracle.procedural_from(r.procedural), obj, glob, oracle.from_params(march),
                                          PW, PH, FMT_RGBA32F)
        a = r.render(PW, PH, FMT_RGBA32F).cpu().numpy()
        deferred = r.get_option("shadow_defer_last")
        mid = r.alloc_target(PW, PH, FMT_RGBA32F)
        r.render_rect(mid, (5, 6, 30, 20), FMT_RGBA32F)
        b = r.render(PW, PH, FMT_RGBA32F).cpu().numpy()
        assert r.get_option("shadow_defer_last") == deferred   # the second render took the first one's path
        assert np.array_equal(a, ref) and np.array_equal(b, ref)
        assert np.array_equal(mid.cpu().numpy()[6:26, 5:35], ref[6:26, 5:35])
    finally:
        r.set_procedural(enabled=0)


# ---- validation ---------------------------------------------------------------------
def test_refusals_write_nothing(r, base):
    osd, gsd = vr.reference_shader_data(FW / FH)
    setup(r, 0, base, osd, gsd)
    buf, view = sentinel_buffer(FMT_RGBA8_UNORM)
    cnt = torch.full((1,), COUNT0, dtype=torch.int64, device="cuda")

    def target(**kw):
        t = _lib.Target(width=FW, height=FH, format=FMT_RGBA8_UNORM, band_rows=0, band_stride=1, band_first=0,
                        pixels=view.data_ptr(), row_pitch=view.stride(0), step_counter=cnt.data_ptr())
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def status(ctx, t, rect):
        tp = ctypes.byref(t) if t is not None else None
        rp = ctypes.byref(_lib.Rect(*rect)) if rect is not None else None
        return _lib.load().vr_render_rect(ctx, tp, rp, None)

    ok = (3, 5, 9, 7)
    bad_rects = [(-1, 5, 9, 7), (3, -1, 9, 7), (3, 5, -9, 7), (3, 5, 9, -7), (60, 5, 8, 7), (3, 40, 9, 6),
                 (FW, 0, 1, 1), (0, FH + 1, 0, 0), (2 ** 31 - 1, 0, 2, 1)]
    for rect in bad_rects:
        assert status(r._ctx, target(), rect) == 1, rect
        assert "vr_render_rect" in _lib.load().vr_last_error().decode()
    bad_targets = [dict(band_rows=8), dict(band_rows=8, band_stride=2, band_flip=1), dict(band_flip=1),
                   dict(format=FMT_RGBA8_UNORM | _lib.TARGET_BANDS_IN_PLACE),
                   dict(format=FMT_RGBA8_UNORM | _lib.TARGET_ROW_RANGE, band_rows=8),
                   dict(format=6), dict(pixels=None), dict(width=0), dict(reserved=1), dict(row_pitch=FW * 4 - 4)]
    for kw in bad_targets:
        assert status(r._ctx, target(**kw), ok) == 1, kw
    assert status(None, target(), ok) == 1
    assert status(r._ctx, None, ok) == 1
    assert status(r._ctx, target(), None) == 1
    with vr.Renderer(0) as fresh:
        fresh.set_shader_data(osd, gsd)
        assert status(fresh._ctx, target(), ok) == 3      # VR_ERR_NO_VOLUME
        rect = _lib.Rect()
        assert _lib.load().vr_update_footprint(fresh._ctx, FW, FH, 0, 0, 0, 1, 1, 1, ctypes.byref(rect)) == 3
    with vr.Renderer(0) as fresh:
        fresh.set_volume(base)
        assert status(fresh._ctx, target(), ok) == 4      # VR_ERR_NO_CAMERA
        assert _lib.load().vr_update_footprint(fresh._ctx, FW, FH, 0, 0, 0, 1, 1, 1, ctypes.byref(rect)) == 4
    for kind, st in ((1, 2), (2, 5)):                     # inject_throw: VR_ERR_HIP / VR_ERR_OOM, as vr_render
        r.set_option("inject_throw", kind)
        with pytest.raises(VRError) as e:
            r.render_rect(view, ok, FMT_RGBA8_UNORM, step_counter=cnt)
        assert e.value.status == st and "vr_render_rect" in str(e.value)
    with pytest.raises(VRError):
        r.update_footprint((NX, 0, 0), (1, 1, 1), FW, FH)
    with pytest.raises(ValueError):                       # the wrapper checks the tensor as render() does
        r.render_rect(view.cpu(), ok, FMT_RGBA8_UNORM)
    torch.cuda.synchronize()
    assert (buf.view(torch.uint8) == 0xA5).all() and int(cnt.item()) == COUNT0
    r.render_rect(view, ok, FMT_RGBA8_UNORM, step_counter=cnt)   # and the accepted call does write
    torch.cuda.synchronize()
    assert int((buf[..., 3] != 0xA5).sum().item()) == 9 * 7   # alpha is 255 in every written pixel
