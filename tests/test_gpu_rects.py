"""vr_render_rects (a list of pixel rectangles in one launch) and the K-edit
loop `update K boxes -> re-render their footprints at once` on the GPU, against
the CPU oracle.  Every comparison is exact and covers the WHOLE buffer: the
oracle's frame inside the union of the rectangles, the sentinel everywhere
else, and the counter equal to its start plus the oracle's per-pixel step
counts summed over the union -- each pixel once, however many rectangles hold
it (a loop over vr_render_rect counts the overlaps again: the duplicate,
contained and overlapping lists catch that on the counter).

Shapes and conventions are those of tests/test_gpu_rect.py: 37 x 22 x 45 random
bytes (seed 20240607), a 67 x 45 frame at 32 steps in a 0xA5-filled buffer with
guard rows and a padded pitch, the counter starting at 1000; the K-edit loop
uses the 64 x 64 frame, camera (0, 0) and three boxes of tests/test_gpu_update.py.

Where the oracle has no per-pixel count -- executed steps under early_out,
density evaluations of the procedural medium (option "count" 1; "count" 2 is
27 Worley cells per evaluation in these kernels) -- it still has them per frame
row (a one-row band), so there the counter is checked exactly on a list of
overlapping full-width rectangles and on the four overlapping quadrants, and
on the overlapping list by inclusion-exclusion over vr_render_rect of the two
rectangles and of their intersection.
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
                                         FMT_RGBA8_UNORM, FMT_RGBA32F)

NX, NY, NZ = 37, 22, 45
STEPS = 32
LAYOUTS = [(1, "planar"), (5, "corner8"), (12, "brick4832"), (14, "cornerh"), (15, "col48")]
LAYOUT_IDS = [n for _, n in LAYOUTS]
UNIFORM_VARIANTS = [(p, n) for p, n in LAYOUTS if p in (12, 14, 15)]   # the layouts with _uX kernels

FW, FH = 67, 45
ALL_FORMATS = (FMT_RGBA32F, FMT_RGBA8_UNORM, FMT_RGBA8_SRGB, FMT_R8_UNORM, FMT_R8_SRGB, FMT_R32F)
GUARD, PAD = 3, 5      # guard rows above and below, padding pixels at the end of each row
COUNT0 = 1000          # the counter's non-zero start

OVERLAP = [(5, 6, 40, 30), (20, 1, 30, 20)]          # across tiles, different anchors
OVERLAP_BOTH = (20, 6, 25, 15)                       # their intersection
ROW_BANDS = [(0, 6, FW, 20), (0, 20, FW, 10), (0, 3, FW, 5), (0, 8, FW, 2)]   # union: rows 3 .. 29, every pixel of them
LISTS = {
    "one_rectangle": [(5, 6, 40, 30)],
    "two_disjoint": [(0, 0, 9, 7), (50, 30, 17, 15)],
    "two_overlapping_in_one_tile": [(3, 5, 4, 2), (5, 6, 4, 4)],
    "overlap_across_tiles": OVERLAP,
    "contained_small_first": [(10, 10, 3, 3), (5, 6, 40, 30)],
    "contained_large_first": [(5, 6, 40, 30), (10, 10, 3, 3)],
    "four_identical": [(3, 5, 9, 7)] * 4,
    "with_empties_between": [(0, 0, 9, 7), (12, 3, 0, 5), (50, 30, 17, 15), (7, 7, 3, 0), (5, 4, 9, 7), (0, 0, 0, 0)],
    "64_columns": [(x, 0, 1, FH) for x in range(64)],
    "64_block_grid": [(3 + 8 * i, 2 + 8 * j, 8, 8) for j in range(8) for i in range(8)
                      if 3 + 8 * i + 8 <= FW and 2 + 8 * j + 8 <= FH],
    "whole_frame_quadrants": [(0, 0, 36, 25), (33, 0, FW - 33, 25), (0, 22, 36, FH - 22), (33, 22, FW - 33, FH - 22)],
    "count_0": [],
    # At this camera the volume's image is x 18 .. 48, y 8 .. 40: the small rectangles above lie on
    # the background, where a pixel counts no step.  The same shapes on the image, so that a pixel
    # counted twice shows on the counter:
    "lit_two_overlapping_in_one_tile": [(25, 17, 4, 2), (27, 18, 4, 4)],
    "lit_contained_small_first": [(30, 20, 3, 3), (5, 6, 40, 30)],
    "lit_contained_large_first": [(5, 6, 40, 30), (30, 20, 3, 3)],
    "lit_four_identical": [(27, 21, 9, 7)] * 4,
}
# the lists that a loop over vr_render_rect gets wrong on the counter
COUNTED_TWICE = ("overlap_across_tiles", "whole_frame_quadrants", "lit_two_overlapping_in_one_tile",
                 "lit_contained_small_first", "lit_contained_large_first", "lit_four_identical")

# the K-edit loop: (origin, extent) of interior_texel, corner_xyz and straddle_5x9x34 of
# tests/test_gpu_update.py, which share the camera (0, 0)
EDIT_BOXES = [((17, 11, 23), (1, 1, 1)), ((NX - 1, NY - 1, NZ - 1), (1, 1, 1)), ((2, 6, 30), (34, 9, 5))]
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
        for a in (f32, u8, n):
            a.setflags(write=False)
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


def union_mask(rects, w=FW, h=FH):
    m = np.zeros((h, w), bool)
    for q in rects:
        x, y, rw, rh = (q.x, q.y, q.width, q.height) if isinstance(q, _lib.Rect) else q
        m[y:y + rh, x:x + rw] = True
    return m


def expect_buffer(buf_shape, dtype, ref, mask):
    """The sentinel buffer with `ref`'s pixels inside the union."""
    e = np.empty(buf_shape, dtype)
    e.view(np.uint8).fill(0xA5)
    h, w = mask.shape
    frame = e[GUARD:GUARD + h, :w]
    frame[mask] = ref[mask]
    return e


def assert_bytes_equal(got, want, what):
    g, w = got.view(np.uint8).reshape(got.shape[0], -1), want.view(np.uint8).reshape(want.shape[0], -1)
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} differing bytes, first (row, byte) {bad[:6].tolist()}"


def new_counter():
    return torch.full((1,), COUNT0, dtype=torch.int64, device="cuda")


def check_list(rr, ref, n, fmt, rects, what, want_count=None):
    """render_rects of the list into a fresh sentinel buffer: the whole buffer
    and the counter afterwards.  n: per-pixel counts (or None with want_count,
    the union's count, or neither: pixels only).  Returns the buffer."""
    h, w = ref.shape[0], ref.shape[1]
    buf, view = sentinel_buffer(fmt, w, h)
    cnt = new_counter()
    rr.render_rects(view, rects, fmt, step_counter=cnt)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    mask = union_mask(rects, w, h)
    assert_bytes_equal(got, expect_buffer(got.shape, got.dtype, ref, mask), f"{what} fmt {fmt}")
    if n is not None:
        want_count = int(n[mask].sum())
    if want_count is not None:
        assert int(cnt.item()) == COUNT0 + want_count, (what, fmt, int(cnt.item()) - COUNT0, want_count)
    return got


def frame_refs(rr, f32, u8):
    """vr_render's frame per format: the oracle's where it is exact, vr_render's
    own for the sRGB formats (the oracle is within 1 LSB there)."""
    own = {fmt: rr.render(FW, FH, fmt).cpu().numpy() for fmt in (FMT_RGBA8_SRGB, FMT_R8_SRGB)}
    assert np.array_equal(own[FMT_RGBA8_SRGB][..., 0], own[FMT_R8_SRGB])
    return {FMT_RGBA32F: f32, FMT_RGBA8_UNORM: u8, FMT_R32F: f32[..., 0], FMT_R8_UNORM: u8[..., 0], **own}


# ---- rectangle lists -------------------------------------------------------------
@pytest.mark.parametrize("lname", list(LISTS))
@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_rect_lists(r, oracle, base, pref, name, lname):
    osd, gsd = vr.reference_shader_data(FW / FH)
    march = vr.march_defaults(max_steps=STEPS)
    setup(r, pref, base, osd, gsd, march)
    assert r.kernel_variant.startswith(f"grid_{name}_clamp"), r.kernel_variant
    f32, u8, steps, n = oracle_refs(oracle, base, osd, gsd, march, FW, FH)
    assert steps == n.sum() > 0
    refs = frame_refs(r, f32, u8)
    # vr_render itself agrees with the oracle here, so "what vr_render writes there" is the oracle's frame
    assert np.array_equal(r.render(FW, FH, FMT_RGBA32F).cpu().numpy(), f32)
    rects = LISTS[lname]
    mask = union_mask(rects)
    if lname in COUNTED_TWICE:   # the case shows something: the rectangles' counts add up to more than the union's
        assert sum(int(n[y:y + h, x:x + w].sum()) for x, y, w, h in rects) > int(n[mask].sum()) > 0
    if lname == "64_block_grid":
        assert len(rects) == 40
    if lname == "whole_frame_quadrants":
        assert mask.all()
    for fmt in ALL_FORMATS if name == "col48" else (FMT_RGBA32F, FMT_RGBA8_SRGB):
        got = check_list(r, refs[fmt], n, fmt, rects, f"{name} {lname}")
        if lname == "one_rectangle":         # the buffer vr_render_rect leaves
            buf, view = sentinel_buffer(fmt)
            r.render_rect(view, rects[0], fmt)
            assert_bytes_equal(got, buf.cpu().numpy(), f"{name} {lname} fmt {fmt} against render_rect")
        if lname == "whole_frame_quadrants":  # the buffer vr_render leaves
            buf, view = sentinel_buffer(fmt)
            r.render(FW, FH, fmt, out=view)
            assert_bytes_equal(got, buf.cpu().numpy(), f"{name} {lname} fmt {fmt} against render")
        if lname == "count_0":
            assert (got.view(np.uint8) == 0xA5).all()


def test_rects_as_structs_and_null_list(r, oracle, base):
    """The wrapper takes vr_rect structs too; count 0 with a NULL list is VR_OK."""
    osd, gsd = vr.reference_shader_data(FW / FH)
    march = vr.march_defaults(max_steps=STEPS)
    setup(r, 15, base, osd, gsd, march)
    f32, _, _, n = oracle_refs(oracle, base, osd, gsd, march, FW, FH)
    check_list(r, f32, n, FMT_RGBA32F, [vr.Rect(*q) for q in OVERLAP], "structs")
    buf, view = sentinel_buffer(FMT_RGBA32F)
    cnt = new_counter()
    t = _lib.Target(width=FW, height=FH, format=FMT_RGBA32F, band_rows=0, band_stride=1, band_first=0,
                    pixels=view.data_ptr(), row_pitch=view.stride(0) * 4, step_counter=cnt.data_ptr())
    assert _lib.load().vr_render_rects(r._ctx, ctypes.byref(t), None, 0, None) == 0
    torch.cuda.synchronize()
    assert (buf.view(torch.uint8) == 0xA5).all() and int(cnt.item()) == COUNT0


# ---- other paths -----------------------------------------------------------------
def row_counts(render_rows_of):
    """Per frame row, what the oracle counts for it: render_rows_of(row) renders
    that row alone (a one-row band) and returns its counts."""
    return np.array([render_rows_of(y) for y in range(FH)], np.int64)


def inclusion_exclusion(rr, fmt):
    """The OVERLAP union's count from vr_render_rect: A + B - (A and B)."""
    total = 0
    for rect, sign in ((OVERLAP[0], 1), (OVERLAP[1], 1), (OVERLAP_BOTH, -1)):
        cnt = new_counter()
        rr.render_rect(sentinel_buffer(fmt)[1], rect, fmt, step_counter=cnt)
        total += sign * (int(cnt.item()) - COUNT0)
    return total


def test_overlap_mirrored_repeat(r, oracle, base):
    osd, gsd = vr.reference_shader_data(FW / FH)
    gsd.media_scroll[0 * 4 + 1] = 1.5    # tap 1: u = 0.8 P + 0.3 along x, past 1: mirrored repeat
    march = vr.march_defaults(max_steps=STEPS)
    setup(r, 1, base, osd, gsd, march)
    assert r.kernel_variant == "grid_planar_mirror"
    f32, _, _, n = oracle_refs(oracle, base, osd, gsd, march, FW, FH)
    check_list(r, f32, n, FMT_RGBA32F, OVERLAP, "mirrored repeat")


@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_overlap_early_out(r, oracle, base, pref, name):
    osd, gsd = vr.reference_shader_data(FW / FH)
    march = vr.march_defaults(max_steps=STEPS, density=16.0, early_out=0.5)
    setup(r, pref, base, osd, gsd, march)
    assert r.kernel_variant.endswith("_early")
    f32, _, steps, n = oracle_refs(oracle, base, osd, gsd, march, FW, FH)
    assert 0 < steps < n.sum(), "early_out stops no ray: the case shows nothing"
    check_list(r, f32, None, FMT_RGBA32F, OVERLAP, f"early_out {name}", inclusion_exclusion(r, FMT_RGBA32F))
    # executed steps per row from the oracle: a list of overlapping full-width rectangles
    obj, glob = vr.shader_data_arrays(osd, gsd)
    m = oracle.from_params(march)
    if "early_rows" not in _refs:   # once for the five layouts
        _refs["early_rows"] = row_counts(lambda y: oracle.render(base, obj, glob, m, FW, FH, FMT_RGBA32F, 1, FH, y)[1])
    rows = _refs["early_rows"]
    assert rows.sum() == steps
    check_list(r, f32, None, FMT_RGBA32F, ROW_BANDS, f"early_out rows {name}", int(rows[3:30].sum()))
    check_list(r, f32, None, FMT_RGBA32F, LISTS["whole_frame_quadrants"], f"early_out frame {name}", steps)


@pytest.mark.parametrize("keeps_uniform", [False, True], ids=["breaks_G", "keeps_G"])
@pytest.mark.parametrize("pref,name", UNIFORM_VARIANTS, ids=[n for _, n in UNIFORM_VARIANTS])
def test_overlap_with_a_uniform_channel(r, oracle, base, pref, name, keeps_uniform):
    """G uniform, an edit queued: the list march loads every channel, leaves the
    pending read-back pending, and the next vr_render still resolves it."""
    vol = base.copy()
    vol[..., 1] = 137
    osd, gsd = vr.reference_shader_data(FW / FH)
    march = vr.march_defaults(max_steps=STEPS)
    setup(r, pref, vol, osd, gsd, march)
    assert r.kernel_variant.endswith("_uG"), r.kernel_variant
    r.render(FW, FH, FMT_RGBA32F)
    origin, (bx, by, bz) = (16, 10, 22), (3, 3, 3)
    box = 255 - vol[origin[2]:origin[2] + bz, origin[1]:origin[1] + by, origin[0]:origin[0] + bx]
    box[..., 1] = 137 if keeps_uniform else 138
    r.update_volume(box, origin)
    patched = vol.copy()
    patched[origin[2]:origin[2] + bz, origin[1]:origin[1] + by, origin[0]:origin[0] + bx] = box
    f32, _, _, n = oracle_refs(oracle, patched, osd, gsd, march, FW, FH)
    before = oracle_refs(oracle, vol, osd, gsd, march, FW, FH)[0]
    assert (f32 != before)[union_mask(OVERLAP)].any(), "the edit changes nothing in the union: the case shows nothing"
    check_list(r, f32, n, FMT_RGBA32F, OVERLAP, f"uniform {name}")
    # the next vr_render resolves the read-back as it does without the list render
    assert np.array_equal(r.render(FW, FH, FMT_RGBA32F).cpu().numpy(), f32)
    assert bool(r.get_option("uniform_mask") & 2) == keeps_uniform
    assert r.kernel_variant.endswith("_uG") == keeps_uniform


PSTEPS = 16


@pytest.mark.parametrize("shadow", [0, 8])
def test_overlap_procedural(r, oracle, shadow):
    osd, gsd = vr.reference_shader_data(FW / FH, 20.0, 15.0)
    march = vr.march_defaults(max_steps=PSTEPS)
    r.set_shader_data(osd, gsd)
    r.set_march(march)
    r.set_procedural(shadow_steps=shadow)
    try:
        obj, glob = vr.shader_data_arrays(osd, gsd)
        m = oracle.from_params(march)
        p = oracle.procedural_from(r.procedural)
        ref, steps, evals = oracle.render_procedural(p, obj, glob, m, FW, FH, FMT_RGBA32F, with_evals=True)
        n = np.maximum(oracle.step_counts(obj, glob, m, FW, FH), 0).astype(np.int64)
        assert steps == n.sum() > 0 and ref[..., 0].max() > 0.0
        assert (evals > steps) == (shadow > 0)
        rows = row_counts(lambda y: oracle.render_procedural(p, obj, glob, m, FW, FH, FMT_RGBA32F, 1, FH, y,
                                                             with_evals=True)[1:])
        assert rows.sum(axis=0).tolist() == [steps, evals]
        # count 2, Worley cells: the rectangle kernels evaluate all 27 cells of every density
        # evaluation (no pruned table; vr_internal.h ProcParams::count_evals)
        rows = np.concatenate([rows, 27 * rows[:, 1:]], axis=1)
        cells = 27 * evals
        for count in (0, 1, 2):
            r.set_option("count", count)
            what = f"procedural shadow {shadow} count {count}"
            check_list(r, ref, n if count == 0 else None, FMT_RGBA32F, OVERLAP, what,
                       inclusion_exclusion(r, FMT_RGBA32F))
            check_list(r, ref, None, FMT_RGBA32F, ROW_BANDS, what + " rows", int(rows[3:30, count].sum()))
            check_list(r, ref, None, FMT_RGBA32F, LISTS["whole_frame_quadrants"], what + " frame",
                       (steps, evals, cells)[count])
    finally:
        r.set_option("count", 0)
        r.set_procedural(enabled=0)


# ---- the context is left as it is --------------------------------------------------
def test_context_untouched_col48(r, oracle, base):
    osd, gsd = vr.reference_shader_data(FW / FH)
    setup(r, 15, base, osd, gsd)
    out = r.alloc_target(FW, FH, FMT_RGBA32F)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    r.render(FW, FH, FMT_RGBA32F, out=out, step_counter=cnt)
    h0 = r.get_option("launch_cache_hits")
    r.render(FW, FH, FMT_RGBA32F, out=out, step_counter=cnt)
    first, c1 = out.cpu().numpy(), int(cnt.item())
    variant, umask, hits = r.kernel_variant, r.get_option("uniform_mask"), r.get_option("launch_cache_hits")
    assert hits == h0 + 1   # the baseline: a repeated render is a hit
    other = r.alloc_target(FW, FH, FMT_RGBA32F)
    r.render_rects(other, OVERLAP, FMT_RGBA32F)
    r.render_rects(out, LISTS["64_block_grid"], FMT_RGBA32F)
    assert (r.kernel_variant, r.get_option("uniform_mask"), r.get_option("launch_cache_hits")) == (variant, umask, hits)
    r.render(FW, FH, FMT_RGBA32F, out=out, step_counter=cnt)
    assert r.get_option("launch_cache_hits") == hits + 1
    assert np.array_equal(out.cpu().numpy(), first) and 2 * int(cnt.item()) == 3 * c1 > 0
    assert (r.kernel_variant, r.get_option("uniform_mask")) == (variant, umask)


def test_context_untouched_sorted_procedural(r, oracle):
    osd, gsd = vr.reference_shader_data(FW / FH, 20.0, 15.0)
    r.set_shader_data(osd, gsd)
    r.set_march(vr.march_defaults(max_steps=PSTEPS))
    r.set_procedural(shadow_steps=3)
    try:
        assert r.kernel_variant == "procedural_shadow"   # the cost-sorted schedule
        c1, c2 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        a = r.render(FW, FH, FMT_RGBA32F, step_counter=c1).cpu().numpy()
        variant, umask, deferred = r.kernel_variant, r.get_option("uniform_mask"), r.get_option("shadow_defer_last")
        mid = r.alloc_target(FW, FH, FMT_RGBA32F)
        r.render_rects(mid, OVERLAP, FMT_RGBA32F)
        b = r.render(FW, FH, FMT_RGBA32F, step_counter=c2).cpu().numpy()
        assert r.get_option("shadow_defer_last") == deferred   # the second render took the first one's path
        assert (r.kernel_variant, r.get_option("uniform_mask")) == (variant, umask)
        assert np.array_equal(a, b) and int(c1.item()) == int(c2.item()) > 0
        mask = union_mask(OVERLAP)
        assert np.array_equal(mid.cpu().numpy()[mask], a[mask])
    finally:
        r.set_procedural(enabled=0)


# ---- validation ---------------------------------------------------------------------
def test_refusals_write_nothing(r, base):
    osd, gsd = vr.reference_shader_data(FW / FH)
    setup(r, 0, base, osd, gsd)
    buf, view = sentinel_buffer(FMT_RGBA8_UNORM)
    cnt = new_counter()
    lib = _lib.load()

    def target(**kw):
        t = _lib.Target(width=FW, height=FH, format=FMT_RGBA8_UNORM, band_rows=0, band_stride=1, band_first=0,
                        pixels=view.data_ptr(), row_pitch=view.stride(0), step_counter=cnt.data_ptr())
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def status(ctx, t, rects, count=None, null=False):
        arr = (_lib.Rect * max(1, len(rects)))(*[_lib.Rect(*q) for q in rects])
        return lib.vr_render_rects(ctx, ctypes.byref(t) if t is not None else None, None if null else arr,
                                   len(rects) if count is None else count, None)

    def refused(st):
        assert st == 1 and "vr_render_rects" in lib.vr_last_error().decode()

    ok = [(3, 5, 9, 7), (20, 10, 5, 5)]
    refused(status(r._ctx, target(), ok, count=-1))
    refused(status(r._ctx, target(), [ok[0]] * 65))
    assert status(r._ctx, target(), [ok[0]] * 64) == 0           # the longest list is taken
    torch.cuda.synchronize()
    assert int((buf[..., 3] != 0xA5).sum().item()) == 9 * 7
    buf.view(torch.uint8).fill_(0xA5)
    cnt.fill_(COUNT0)
    refused(status(r._ctx, target(), ok, count=1, null=True))
    refused(status(r._ctx, target(), ok + [(60, 40, 8, 5)]))      # the last of three leaves the frame by one pixel
    refused(status(r._ctx, target(), ok + [(60, 40, 7, 6)]))
    for bad in ((-1, 5, 9, 7), (3, -1, 9, 7), (3, 5, -9, 7), (3, 5, 9, -7), (FW, 0, 1, 1), (0, FH + 1, 0, 0),
                (2 ** 31 - 1, 0, 2, 1)):
        refused(status(r._ctx, target(), [ok[0], bad, ok[1]]))
    bad_targets = [dict(band_rows=8), dict(band_rows=8, band_stride=2, band_flip=1), dict(band_flip=1),  # band targets
                   dict(format=FMT_RGBA8_UNORM | _lib.TARGET_ROW_RANGE, band_rows=8),                   # a row range
                   dict(format=FMT_RGBA8_UNORM | _lib.TARGET_BANDS_IN_PLACE),                           # in place
                   dict(format=6), dict(pixels=None), dict(width=0), dict(reserved=1), dict(row_pitch=FW * 4 - 4)]
    for kw in bad_targets:
        refused(status(r._ctx, target(**kw), ok))
    refused(status(None, target(), ok))
    refused(status(r._ctx, None, ok))
    with vr.Renderer(0) as fresh:
        fresh.set_shader_data(osd, gsd)
        assert status(fresh._ctx, target(), ok) == 3      # VR_ERR_NO_VOLUME
    with vr.Renderer(0) as fresh:
        fresh.set_volume(base)
        assert status(fresh._ctx, target(), ok) == 4      # VR_ERR_NO_CAMERA
    for kind, st in ((1, 2), (2, 5)):                     # inject_throw: VR_ERR_HIP / VR_ERR_OOM, as vr_render
        r.set_option("inject_throw", kind)
        with pytest.raises(vr.VRError) as e:
            r.render_rects(view, ok, FMT_RGBA8_UNORM, step_counter=cnt)
        assert e.value.status == st and "vr_render_rects" in str(e.value)
    with pytest.raises(ValueError):                       # the wrapper checks the tensor as render() does
        r.render_rects(view.cpu(), ok, FMT_RGBA8_UNORM)
    torch.cuda.synchronize()
    assert (buf.view(torch.uint8) == 0xA5).all() and int(cnt.item()) == COUNT0
    r.render_rects(view, ok, FMT_RGBA8_UNORM, step_counter=cnt)   # and the accepted call does write
    torch.cuda.synchronize()
    assert int((buf[..., 3] != 0xA5).sum().item()) == 9 * 7 + 5 * 5   # alpha is 255 in every written pixel


# ---- the K-edit loop ------------------------------------------------------------------
def patch_into(vol, box, origin):
    x0, y0, z0 = origin
    bz, by, bx, _ = box.shape
    out = vol.copy()
    out[z0:z0 + bz, y0:y0 + by, x0:x0 + bx] = box
    return out


@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_k_edit_loop(r, oracle, base, pref, name):
    """Render whole, update three boxes, update_footprints, ONE render_rects:
    the buffer is the oracle's frame of the patched volume, byte for byte."""
    osd, gsd = vr.reference_shader_data(1.0, 0.0, 0.0)
    march = vr.march_defaults(max_steps=STEPS)
    rng = np.random.default_rng(20240621)
    boxes = [rng.integers(0, 256, size=(bz, by, bx, 4), dtype=np.uint8) for _, (bx, by, bz) in EDIT_BOXES]
    before = oracle_refs(oracle, base, osd, gsd, march, EW, EH)[0]
    patched = base
    for (origin, _), box in zip(EDIT_BOXES, boxes):
        alone = oracle_refs(oracle, patch_into(base, box, origin), osd, gsd, march, EW, EH)[0]
        assert (alone != before).any(), f"the edit at {origin} changes no pixel: the case shows nothing"
        patched = patch_into(patched, box, origin)
    want = oracle_refs(oracle, patched, osd, gsd, march, EW, EH)[0]
    fps_cpu = [vr.volume_box_footprint(osd, gsd, march, (NX, NY, NZ), o, e, EW, EH) for o, e in EDIT_BOXES]
    assert 0 < union_mask(fps_cpu, EW, EH).sum() < EW * EH, "the footprints cover the frame: the case shows nothing"

    setup(r, pref, base, osd, gsd, march)
    assert r.kernel_variant.startswith(f"grid_{name}_clamp"), r.kernel_variant
    buf, frame = sentinel_buffer(FMT_RGBA32F, EW, EH)
    r.render(EW, EH, FMT_RGBA32F, out=frame)
    for (origin, _), box in zip(EDIT_BOXES, boxes):
        r.update_volume(box, origin)
    fps = r.update_footprints(EDIT_BOXES, EW, EH)
    assert fps == fps_cpu
    r.render_rects(frame, fps, FMT_RGBA32F)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert_bytes_equal(got, expect_buffer(got.shape, got.dtype, want, np.ones((EH, EW), bool)), f"K-edit loop {name}")
