"""vr_query_rect (per-pixel ray records) on the GPU.  Every comparison but one
is exact: steps against the oracle's per-pixel step counts, `value` against
vr_render's R32F pixel bit for bit, the hit against the existing early-out
march, the hit point against numpy float32 additions.  The one tolerance
(entry / step against the float64 reading of tests/glsl_f64.py) is stated at
ENTRY_STEP_TOL.

Shapes: the 16^3 golden volume and a 32 x 24 x 16 random one (no two axes
alike), a 64 x 48 frame, 32 steps, the reference camera at two angles (both
leave most of the frame uncovered: the -1 records), the rectangles
(5, 3, 43, 37) -- unaligned, partial 8 x 8 tiles on all four sides -- and the
whole frame.  Procedural medium: 48 x 40, 16 steps.

The hit cases run at march.density = 32 (grid) and 64 (procedural), chosen on
the CPU oracle: at density 32 and threshold 0.5, 43 % to 79 % of the covered
pixels of these volumes and cameras end below the threshold (so have a hit) and
the rest do not; the oracle's early-out step total drops from ~7950 to
2700 - 5300.  test_hit_matches_the_early_out_march re-checks that condition
from the oracle's frame before it looks at the GPU's answer.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd import _lib  # noqa: E402
from volumetricrenderer_amd._lib import FMT_R32F, FMT_RGBA32F, VRError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, STEPS = 64, 48, 32
RECT, WHOLE = (5, 3, 43, 37), (0, 0, W, H)
CAMERAS = [(0.0, 0.0), (40.0, 25.0)]
# every built layout, and the planar march under both wraps (a MediaScroll that leaves [0, 1] forces mirrored repeat)
LAYOUTS = [(1, "planar", False), (1, "planar_mirror", True), (5, "corner8", False), (12, "brick4832", False),
           (14, "cornerh", False), (15, "col48", False)]
LAYOUT_IDS = [n for _, n, _ in LAYOUTS]
HIT_DENSITY = 32.0        # see the module docstring
PROC_HIT_DENSITY = 64.0   # the procedural medium: 55 % of the covered pixels end below 0.5
THRESHOLDS = (0.9, 0.5, 0.1)
# Case 5.  Largest |entry - f64| and |step - f64| over both cameras, measured on an MI355X at these
# shapes: 7.904e-7 (entry, camera (40, 25); 4.384e-7 at (0, 0)) and 7.666e-9 (step) -- the fp32 ray
# setup's few ulps, on values in [0, 1], of a ray that starts 5.2 units away.  The assertion is four
# times the larger one, for headroom over other cameras; half a texel of the 32-texel axis
# (0.5 / 32 = 0.0156), beyond which a hit no longer names a texel, is almost four orders above it.
ENTRY_STEP_MEASURED = 7.904e-7
ENTRY_STEP_TOL = 4 * ENTRY_STEP_MEASURED
assert ENTRY_STEP_TOL < 0.5 / 32
SENTINEL = 0x5A5A5A5A
PW, PH, PSTEPS = 48, 40, 16


@pytest.fixture(scope="module")
def volumes():
    return {"golden16": np.load(os.path.join(ROOT, "tests", "golden", "volume16_literal.npy")),
            "random32x24x16": np.random.default_rng(20241020).integers(0, 256, size=(16, 24, 32, 4), dtype=np.uint8)}


@pytest.fixture(scope="module")
def r():
    with vr.Renderer(0) as rr:
        yield rr


def camera(angles, mirror=False, aspect=W / H):
    osd, gsd = vr.reference_shader_data(aspect, *angles)
    if mirror:
        gsd.media_scroll[0 * 4 + 1] = 1.5    # tap 1: u = 0.8 P + 0.3 along x, past 1
        gsd.media_scroll[1 * 4 + 2] = -1.0   # tap 2: u from -0.25 along y
    return osd, gsd


def setup(rr, pref, vol, osd, gsd, **march):
    rr.set_procedural(enabled=0)
    rr.set_option("uniform_skip", 1)
    rr.set_option("count", 0)
    rr.set_layout_preference(pref)
    rr.set_volume(vol)
    rr.set_shader_data(osd, gsd)
    rr.set_march(vr.march_defaults(max_steps=STEPS, **march))


def expect_variant(rr, name):
    want = "grid_planar_mirror" if name == "planar_mirror" else f"grid_{name}_clamp"
    assert rr.kernel_variant.startswith(want), rr.kernel_variant


def query(rr, rect, threshold=0.0, w=W, h=H):
    rec = vr.ray_records(rr.query_rect(rect, w, h, threshold))
    assert rec.shape == (rect[3], rect[2])
    return rec


def oracle_steps(oracle, osd, gsd, march, w=W, h=H):
    obj, glob = vr.shader_data_arrays(osd, gsd)
    return oracle.step_counts(obj, glob, oracle.from_params(march), w, h)


def crop(a, rect):
    x, y, w, h = rect
    return a[y:y + h, x:x + w]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def hit_relation(a_rec, b_rec, what):
    """Case 3 at one threshold: query A (context early_out 0, threshold T) gives h and n, query B
    (context early_out T, threshold 0) gives s.  h >= 0 -> s == h + 1; h == -1 -> s == n."""
    h, n, s = a_rec["hit_step"], a_rec["steps"], b_rec["steps"]
    cov = n >= 0
    assert np.array_equal(cov, s >= 0), what
    assert (h[~cov] == -1).all() and (h[cov] < n[cov]).all() and (h >= -1).all(), what
    hit = cov & (h >= 0)
    miss = cov & (h < 0)
    bad = np.argwhere(hit & (s != h + 1))
    assert bad.size == 0, f"{what}: s != h + 1 at (y, x) {bad[:6].tolist()}"
    bad = np.argwhere(miss & (s != n))
    assert bad.size == 0, f"{what}: no hit but s != n at (y, x) {bad[:6].tolist()}"
    assert (b_rec["hit_step"] == -1).all(), what   # threshold 0: no search
    return hit, miss


# ---- 1. steps ------------------------------------------------------------------------
@pytest.mark.parametrize("pref,name,mirror", LAYOUTS, ids=LAYOUT_IDS)
def test_steps_match_the_oracle(r, oracle, volumes, pref, name, mirror):
    uncovered = 0
    for vname, vol in volumes.items():
        for angles in CAMERAS:
            osd, gsd = camera(angles, mirror)
            setup(r, pref, vol, osd, gsd)
            expect_variant(r, name)
            n = oracle_steps(oracle, osd, gsd, r.march)
            rec = query(r, WHOLE)
            assert np.array_equal(rec["steps"], n), (vname, angles)   # the -1 entries included
            uncovered += int((n < 0).sum())
            assert (n == 0).any() and n.max() > 8                     # covered rays of zero steps, and long ones
            part = query(r, RECT)
            assert np.array_equal(part["steps"], crop(n, RECT))
            cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
            r.render_rect(r.alloc_target(W, H, FMT_R32F), RECT, FMT_R32F, step_counter=cnt)
            assert int(part["steps"][part["steps"] >= 0].sum()) == int(cnt.item()) > 0
    assert uncovered > 0


# ---- 2. value and optical depth --------------------------------------------------------
@pytest.mark.parametrize("pref,name,mirror", LAYOUTS, ids=LAYOUT_IDS)
def test_value_is_the_render_and_follows_from_optical_depth(r, oracle, volumes, pref, name, mirror):
    expf = oracle.lib().vro_expf
    for vname, vol in volumes.items():
        for angles in CAMERAS:
            osd, gsd = camera(angles, mirror)
            setup(r, pref, vol, osd, gsd)
            frame = r.render(W, H, FMT_R32F).cpu().numpy()
            assert frame.max() > 0.0
            for rect in (RECT, WHOLE):
                rec = query(r, rect)
                assert np.array_equal(bits(rec["value"]), bits(crop(frame, rect))), (vname, angles, rect)
            cov = rec["steps"] >= 0
            d = np.float32(r.march.density)
            od = rec["optical_depth"][cov]
            arg = d * np.minimum(-od, np.float32(0.0))
            assert arg.dtype == np.float32
            want = np.float32(1.0) - np.array([expf(float(v)) for v in arg], np.float32)   # frag.glsl:79
            assert np.array_equal(bits(want), bits(rec["value"][cov])), (vname, angles)
            assert (rec["value"][~cov] == 0).all() and (rec["optical_depth"][~cov] == 0).all()


# ---- 3. the hit against the existing early-out march -------------------------------------
@pytest.mark.parametrize("pref,name,mirror", LAYOUTS, ids=LAYOUT_IDS)
def test_hit_matches_the_early_out_march(r, oracle, volumes, pref, name, mirror):
    for vname, vol in volumes.items():
        osd, gsd = camera(CAMERAS[1], mirror)
        obj, glob = vr.shader_data_arrays(osd, gsd)
        # the condition, from the oracle alone: at threshold 0.5 a quarter of the covered rays end below
        # it (transmittance = 1 - value; the accumulator only grows), at least one does not, and the
        # oracle's early-out march executes fewer steps
        m0 = vr.march_defaults(max_steps=STEPS, density=HIT_DENSITY)
        ref, total = oracle.render(vol, obj, glob, oracle.from_params(m0), W, H, FMT_RGBA32F)
        n = oracle_steps(oracle, osd, gsd, m0)
        below = ref[..., 0][n >= 0] > 0.5
        _, total_early = oracle.render(vol, obj, glob, oracle.from_params(
            vr.march_defaults(max_steps=STEPS, density=HIT_DENSITY, early_out=0.5)), W, H, FMT_RGBA32F)
        print(f"{vname}: {below.mean():.3f} of {below.size} covered rays end below 0.5; steps {total} -> {total_early}")
        assert below.mean() >= 0.25 and not below.all() and total_early < total
        for tau in THRESHOLDS:
            setup(r, pref, vol, osd, gsd, density=HIT_DENSITY)
            expect_variant(r, name)
            a = query(r, RECT, tau)
            setup(r, pref, vol, osd, gsd, density=HIT_DENSITY, early_out=tau)
            assert r.kernel_variant.endswith("_early")
            b = query(r, RECT, 0.0)
            hit, miss = hit_relation(a, b, f"{name} {vname} threshold {tau}")
            if tau == 0.5:
                assert hit.sum() >= 0.25 * (hit.sum() + miss.sum()) and miss.any()
                grey = crop(ref[..., 0], RECT)
                clear = np.abs(grey - 0.5) > 1e-4     # away from the threshold itself, where fp32 rounding decides
                assert np.array_equal(hit[clear], (crop(n >= 0, RECT) & (grey > 0.5))[clear])
            # the context's own early_out ends the search: with both set, the looser one stops the ray first
            both = query(r, RECT, 0.1)
            assert np.array_equal(both["steps"], b["steps"])
            assert ((both["hit_step"] == -1) | (both["hit_step"] == both["steps"] - 1)).all()
            if tau > 0.1:
                assert (both["hit_step"] == -1).sum() >= (a["hit_step"] == -1).sum()


# ---- 4. the hit point ----------------------------------------------------------------------
@pytest.mark.parametrize("pref,name,mirror", LAYOUTS, ids=LAYOUT_IDS)
def test_hit_point_is_entry_plus_steps_in_fp32(r, volumes, pref, name, mirror):
    osd, gsd = camera(CAMERAS[0], mirror)
    setup(r, pref, volumes["random32x24x16"], osd, gsd, density=HIT_DENSITY)
    raw = r.query_rect(WHOLE, W, H, 0.5)
    rec = vr.ray_records(raw)
    h = rec["hit_step"]
    assert (h >= 0).sum() > 100 and h.max() >= 2
    p = rec["entry"].astype(np.float32).copy()
    want = np.zeros_like(p)
    for i in range(int(h.max()) + 1):      # P_i = (...((entry + step) + step)...), never entry + i * step
        at = h == i
        want[at] = p[at]
        p = (p + rec["step"]).astype(np.float32)
    assert np.array_equal(bits(want), bits(rec["hit"]))
    assert (rec["hit"][h < 0] == 0).all()
    words = raw.cpu().numpy()
    assert (words[..., [7, 11, 15]] == 0).all()   # the reserved words
    assert (rec["reserved0"] == 0).all() and (rec["reserved1"] == 0).all() and (rec["reserved2"] == 0).all()
    cov = rec["steps"] >= 0
    assert (words[~cov][:, 2:] == 0).all() and (words[~cov][:, :2] == -1).all()
    inside = rec["hit"][h >= 0]
    assert (inside >= -1e-5).all() and (inside <= 1 + 1e-5).all()   # a sample point of the box


# ---- 5. entry and step against the independent float64 reading -----------------------------
def f64_entry_and_step(monkeypatch, vol, osd, gsd, march):
    """Pin and stepVec of tests/glsl_f64.py's own ray setup: its march hands tap 0 the ray point
    itself (scale 1, weight 0: u = P), so the first two calls for channel 0 carry P_0 and P_1."""
    import glsl_f64
    seen = []

    def record(vol_c, nx, ny, nz, u):
        seen.append(u.copy())
        return np.zeros(u.shape[0])

    assert march.tap_scale[0] == 1.0 and march.tap_weight[0] == 0.0
    monkeypatch.setattr(glsl_f64, "_texture", record)
    obj, glob = vr.shader_data_arrays(osd, gsd)
    _, n = glsl_f64.render(vol, obj, glob, march, W, H)
    p0, p1 = seen[0], seen[4]                  # step 0 tap 0, step 1 tap 0
    idx = np.nonzero(n.ravel() > 0)[0]
    assert len(p0) == idx.size
    two = n.ravel()[idx] > 1
    assert len(p1) == two.sum()
    return n, idx, p0, idx[two], p1 - p0[two]


@pytest.mark.parametrize("angles", CAMERAS, ids=["phi0", "phi40_theta25"])
def test_entry_and_step_match_the_float64_reading(r, volumes, monkeypatch, angles):
    vol = volumes["golden16"]
    osd, gsd = camera(angles)
    setup(r, 0, vol, osd, gsd)
    rec = query(r, WHOLE)
    n, idx, entry, idx2, step = f64_entry_and_step(monkeypatch, vol, osd, gsd, r.march)
    got_n = rec["steps"].ravel()
    both = got_n[idx] > 0                      # the two readings may cut a ray's last step differently
    both2 = got_n[idx2] > 1
    assert both.sum() > 500 and both2.sum() > 500
    de = np.abs(rec["entry"].reshape(-1, 3)[idx][both].astype(np.float64) - entry[both]).max()
    ds = np.abs(rec["step"].reshape(-1, 3)[idx2][both2].astype(np.float64) - step[both2]).max()
    print(f"camera {angles}: max |entry - f64| {de:.3e}, max |step - f64| {ds:.3e} (bound {ENTRY_STEP_TOL:.3e})")
    assert de <= ENTRY_STEP_TOL and ds <= ENTRY_STEP_TOL


# ---- 6. the loop closes: pick -> edit -> footprint -> re-render -------------------------------
@pytest.mark.parametrize("pref,name,mirror", [lay for lay in LAYOUTS if not lay[2]],
                         ids=[n for _, n, m in LAYOUTS if not m])
def test_pick_edit_footprint_rerender(r, oracle, volumes, pref, name, mirror):
    vol = volumes["random32x24x16"]
    nz, ny, nx, _ = vol.shape
    osd, gsd = camera(CAMERAS[1])
    setup(r, pref, vol, osd, gsd, density=HIT_DENSITY)
    px, py = W // 2, H // 2
    rec, texel = r.pick(px, py, W, H, 0.5)
    assert rec["hit_step"] >= 0 and texel is not None
    want_texel = tuple(int(min(max(np.floor(float(rec["hit"][k]) * d), 0), d - 1)) for k, d in enumerate((nx, ny, nz)))
    assert texel == want_texel
    none_rec, none_texel = r.pick(0, 0, W, H, 0.5)          # a corner pixel: not covered
    assert none_rec["steps"] == -1 and none_texel is None
    frame = r.render(W, H, FMT_RGBA32F)
    origin = tuple(min(t, d - 2) for t, d in zip(texel, (nx, ny, nz)))
    box = np.full((2, 2, 2, 4), 255, np.uint8)
    r.update_volume(box, origin)
    fx, fy, fw, fh = r.update_footprint(origin, (2, 2, 2), W, H)
    assert fx <= px < fx + fw and fy <= py < fy + fh
    r.render_rect(frame, (fx, fy, fw, fh), FMT_RGBA32F)
    torch.cuda.synchronize()
    patched = vol.copy()
    x0, y0, z0 = origin
    patched[z0:z0 + 2, y0:y0 + 2, x0:x0 + 2] = 255
    obj, glob = vr.shader_data_arrays(osd, gsd)
    want, _ = oracle.render(patched, obj, glob, oracle.from_params(r.march), W, H, FMT_RGBA32F)
    before, _ = oracle.render(vol, obj, glob, oracle.from_params(r.march), W, H, FMT_RGBA32F)
    assert want[py, px, 0] != before[py, px, 0], "the edit does not change the picked pixel"
    assert frame.cpu().numpy().tobytes() == want.tobytes()
    assert r.render(W, H, FMT_RGBA32F).cpu().numpy().tobytes() == want.tobytes()


# ---- 7. nothing else is touched ----------------------------------------------------------------
def sentinel_records(rows, cols):
    return torch.full((rows, cols, 16), SENTINEL, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("pref,name,mirror", [LAYOUTS[0], LAYOUTS[4], LAYOUTS[5]], ids=["planar", "cornerh", "col48"])
def test_query_writes_its_records_and_nothing_else(r, volumes, pref, name, mirror):
    osd, gsd = camera(CAMERAS[0])
    setup(r, pref, volumes["random32x24x16"], osd, gsd)
    out = r.alloc_target(W, H, FMT_RGBA32F)
    r.render(W, H, FMT_RGBA32F, out=out)
    h0 = r.get_option("launch_cache_hits")
    r.render(W, H, FMT_RGBA32F, out=out)
    before, variant, hits = out.cpu().numpy().tobytes(), r.kernel_variant, r.get_option("launch_cache_hits")
    cached = hits - h0                                       # 1 where a repeated render is a cache hit
    assert cached in (0, 1)
    x, y, w, h = RECT
    guard, pad = 2, 5
    buf = sentinel_records(h + 2 * guard, w + pad)
    view = buf[guard:guard + h, :w]
    assert view.stride(0) == (w + pad) * 16                  # a pitch wider than the rectangle
    r.query_rect(RECT, W, H, 0.5, out=view)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:guard] == SENTINEL).all() and (got[guard + h:] == SENTINEL).all()   # the guard rows
    assert (got[guard:guard + h, w:] == SENTINEL).all()                              # the pad records
    assert np.array_equal(got[guard:guard + h, :w], r.query_rect(RECT, W, H, 0.5).cpu().numpy())
    assert r.get_option("launch_cache_hits") == hits and r.kernel_variant == variant
    r.render(W, H, FMT_RGBA32F, out=out)
    assert r.get_option("launch_cache_hits") == hits + cached   # the cached launch is still there
    assert out.cpu().numpy().tobytes() == before and r.kernel_variant == variant
    # an empty rectangle is accepted and writes nothing
    buf.fill_(SENTINEL)
    for empty in ((10, 10, 0, 5), (10, 10, 5, 0)):
        assert _lib.load().vr_query_rect(r._ctx, W, H, ctypes.byref(_lib.Rect(*empty)), 0.0, buf.data_ptr(), 0,
                                         None) == 0
    assert r.query_rect((3, 3, 0, 0), W, H).shape == (0, 0, 16)
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()


# ---- 8. the procedural medium --------------------------------------------------------------------
@pytest.mark.parametrize("shadow", [0, 2])
def test_procedural_query(r, shadow):
    osd, gsd = vr.reference_shader_data(PW / PH, 20.0, 15.0)
    rect, whole = (3, 5, 30, 21), (0, 0, PW, PH)
    r.set_shader_data(osd, gsd)
    r.set_march(vr.march_defaults(max_steps=PSTEPS, density=PROC_HIT_DENSITY))
    r.set_procedural(shadow_steps=shadow)
    try:
        frame = r.render(PW, PH, FMT_R32F).cpu().numpy()
        assert frame.max() > 0.0
        a = query(r, whole, 0.5, PW, PH)
        assert np.array_equal(bits(a["value"]), bits(frame))
        part = query(r, rect, 0.0, PW, PH)
        assert np.array_equal(bits(part["value"]), bits(crop(frame, rect)))
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        r.render_rect(r.alloc_target(PW, PH, FMT_R32F), rect, FMT_R32F, step_counter=cnt)
        assert int(part["steps"][part["steps"] >= 0].sum()) == int(cnt.item()) > 0
        r.set_option("count", 1)               # density evaluations: the query still counts ray-steps
        assert np.array_equal(query(r, rect, 0.0, PW, PH)["steps"], part["steps"])
        r.set_option("count", 0)
        # optical depth is the view ray's: transmittance exp(-density * od) against the threshold
        cov = a["steps"] >= 0
        t = np.exp(-np.float64(PROC_HIT_DENSITY) * a["optical_depth"].astype(np.float64))
        clear = np.abs(t - 0.5) > 1e-4
        assert np.array_equal((a["hit_step"] >= 0)[cov & clear], (t < 0.5)[cov & clear])
        r.set_march(vr.march_defaults(max_steps=PSTEPS, density=PROC_HIT_DENSITY, early_out=0.5))
        b = query(r, whole, 0.0, PW, PH)
        hit, miss = hit_relation(a, b, f"procedural shadow {shadow}")
        assert hit.sum() > 100 and miss.sum() > 100
        p = a["entry"].copy()
        want = np.zeros_like(p)
        for i in range(int(a["hit_step"].max()) + 1):
            want[a["hit_step"] == i] = p[a["hit_step"] == i]
            p = (p + a["step"]).astype(np.float32)
        assert np.array_equal(bits(want), bits(a["hit"]))
    finally:
        r.set_option("count", 0)
        r.set_procedural(enabled=0)


# ---- 9. refusals ---------------------------------------------------------------------------------
def test_refusals_write_nothing(r, volumes):
    vol = volumes["golden16"]
    osd, gsd = camera(CAMERAS[0])
    setup(r, 0, vol, osd, gsd)
    x, y, w, h = RECT
    buf = sentinel_records(h + 2, w + 3)
    ptr, pitch = buf[1:, 1:].data_ptr(), w + 3
    f = _lib.load().vr_query_rect

    def status(ctx=r._ctx, size=(W, H), rect=RECT, threshold=0.0, d=ptr, p=pitch):
        rp = ctypes.byref(_lib.Rect(*rect)) if rect is not None else None
        return f(ctx, size[0], size[1], rp, threshold, d, p, None)

    bad_rects = [(-1, 3, 43, 37), (5, -1, 43, 37), (5, 3, -43, 37), (5, 3, 43, -37), (30, 3, 35, 37), (5, 20, 43, 29),
                 (W, 0, 1, 1), (0, H + 1, 0, 0), (2 ** 31 - 1, 0, 2, 1)]
    for rect in bad_rects:
        assert status(rect=rect) == 1, rect
        assert "vr_query_rect" in _lib.load().vr_last_error().decode()
    for kw in (dict(ctx=None), dict(rect=None), dict(d=None), dict(size=(0, H)), dict(size=(W, -1)), dict(p=w - 1),
               dict(p=1), dict(d=ptr + 4), dict(threshold=1.0), dict(threshold=-0.25), dict(threshold=float("nan")),
               dict(threshold=2.0)):
        assert status(**kw) == 1, kw
    r.set_march(vr.march_defaults(max_steps=STEPS, density=0.0))
    assert status(threshold=0.5) == 1              # a threshold needs density > 0, as early_out does
    r.set_march(vr.march_defaults(max_steps=STEPS))
    with vr.Renderer(0) as fresh:
        fresh.set_shader_data(osd, gsd)
        assert status(ctx=fresh._ctx) == 3         # VR_ERR_NO_VOLUME
    with vr.Renderer(0) as fresh:
        fresh.set_volume(vol)
        assert status(ctx=fresh._ctx) == 4         # VR_ERR_NO_CAMERA
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()
    with pytest.raises(ValueError):                # the wrapper checks the tensor it is handed
        r.query_rect(RECT, W, H, out=buf[:, :, :8])
    with pytest.raises(ValueError):
        r.query_rect(RECT, W, H, out=buf[:h - 1])
    good = r.query_rect(RECT, W, H, 0.5).cpu().numpy()
    for kind, st in ((1, 2), (2, 5)):              # inject_throw: VR_ERR_HIP / VR_ERR_OOM, as vr_render
        r.set_option("inject_throw", kind)
        with pytest.raises(VRError) as e:
            r.query_rect(RECT, W, H, 0.5, out=buf[1:1 + h, :w])
        assert e.value.status == st and "vr_query_rect" in str(e.value)
        torch.cuda.synchronize()
        assert (buf == SENTINEL).all()
        assert np.array_equal(r.query_rect(RECT, W, H, 0.5).cpu().numpy(), good)   # and it queries exactly again
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()
    r.query_rect(RECT, W, H, 0.5, out=buf[1:1 + h, :w])   # and the accepted call does write
    assert np.array_equal(buf[1:1 + h, :w].cpu().numpy(), good)
