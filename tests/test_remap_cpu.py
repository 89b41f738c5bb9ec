"""vr_remap's host side, the checks that need no GPU: the conditions the shared
inputs must meet; vr_brush_remap_apply against the numpy restatement
(tests/remap_spec.py) on every brush of paint_spec.BRUSHES x table x op x
falloff; vr_lut_levels over its whole argument space; vr_lut_compose with
aliasing; vr_stats_lut on empty, one-bin, two-bin, 2^31 - 1 and real
histograms; invert twice; the identity; refusals; prototypes and exports.
Everything is exact."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clone_spec as cs  # noqa: E402
import paint_spec as ps  # noqa: E402
from brush_harness import base  # noqa: E402,F401
import remap_spec as rs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRENGTHS = [cs.STRENGTH, rs.ZERO_CHANNEL]
OUT_PAIRS = [(0, 255), (255, 0), (10, 240), (240, 10), (7, 7), (200, 3), (0, 1)]


def brush(centre, radius, op=ps.SET, falloff=0, strength=cs.STRENGTH):
    import volumetricrenderer_amd as vr
    return vr.make_brush(centre, radius, op, falloff, (1, 2, 3, 4), strength)


@pytest.fixture(scope="module")
def skewed():
    return rs.skewed_volume()


def assert_exact(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} mismatches, first {bad[:5].tolist()}"


def host_stats(hist):
    import volumetricrenderer_amd as vr
    hist = np.asarray(hist, np.uint64)
    return vr.Stats(int(hist[0].sum()), 256 * int(hist[0].sum()), np.zeros(4, np.uint64), hist)


def test_the_inputs_tell_wrong_implementations_apart(base, skewed):
    """Asserted before anything is compared with the library."""
    T = rs.TABLES
    perm, ident = T["perm"].astype(np.int64), T["identity"].astype(np.int64)
    # perm: four different permutations without a fixed point; the channels cannot be swapped unnoticed (a
    # `c * 256` slip), and a texel remapped twice is seen
    for c in range(4):
        assert sorted(perm[c]) == list(range(256)) and (perm[c] != ident[c]).all()
        for d in range(c + 1, 4):
            assert (perm[c] != perm[d]).sum() > 200
    centre, radius = ps.BRUSHES["whole"]
    want = rs.spec_remap(base, T["perm"], centre, radius, ps.SET, 0, rs.FULL)
    for c in range(3):
        swapped = T["perm"].copy()
        swapped[[c, c + 1]] = swapped[[c + 1, c]]
        assert (rs.spec_remap(base, swapped, centre, radius, ps.SET, 0, rs.FULL) != want).any(), c
    for c in range(4):
        assert (perm[c][perm[c]] != perm[c]).sum() >= 200
        common = np.argsort(np.bincount(base[..., c].ravel(), minlength=256))[-8:]
        assert (perm[c][common] != common).all()
    twice = rs.spec_remap(want, T["perm"], centre, radius, ps.SET, 0, rs.FULL)
    assert (twice != want).mean() > 0.9
    # the skewed volume: G constant (the single-bin rule), the others confined and skewed
    assert (skewed[..., 1] == rs.SKEW_G).all()
    for c, (lowest, span) in rs.SKEW_RANGE.items():
        ch = skewed[..., c]
        assert ch.min() == lowest and ch.max() == lowest + span and np.median(ch) < lowest + span // 3
    for c in (0, 2, 3):
        assert (T["eq"][c] != ident[c]).sum() >= 64 and (T["eq"][c] != T["stretch"][c]).sum() >= 64
        assert (T["stretch"][c] != ident[c]).sum() >= 64
    assert (T["eq"][1] == ident[1]).all() and (T["stretch"][1] == ident[1]).all()
    # the named level tables are what their names say
    assert (T["invert"] == 255 - ident).all()
    assert (T["thresh128"] == np.where(ident >= 128, 255, 0)).all()
    assert T["levels_narrow"][0][40] == 10 and T["levels_narrow"][0][90] == 240 and T["levels_narrow"][0][65] == 125
    assert (T["posterise"] == (ident & 0xC0)).all()
    # every table but the identity changes the base volume under SET
    for name, t in T.items():
        changed = (rs.spec_remap(base, t, centre, radius, ps.SET, 0, rs.FULL) != base).any()
        assert changed == (name != "identity"), name


def test_the_library_builds_the_named_tables(skewed):
    """The library's builders give the specification's tables: the named ones are then used as plain bytes."""
    import volumetricrenderer_amd as vr
    T = rs.TABLES
    assert_exact(vr.lut_identity(), T["identity"])
    assert_exact(vr.lut_levels(0, 255, 255, 0), T["invert"])
    assert_exact(vr.lut_levels(127, 128, 0, 255), T["thresh128"])
    assert_exact(vr.lut_levels(40, 90, 10, 240), T["levels_narrow"])
    centre, radius = ps.BRUSHES[rs.STATS_BRUSH[0]]
    st = vr.brush_stats_host(brush(centre, radius, ps.SET, rs.STATS_BRUSH[1], rs.FULL), skewed)
    assert_exact(st.hist.astype(np.int64), rs.spec_hist(skewed, centre, radius))
    assert_exact(vr.stats_lut(st, vr.LUT_EQUALIZE), T["eq"])
    assert_exact(vr.stats_lut(st, vr.LUT_STRETCH), T["stretch"])
    assert (vr.LUT_EQUALIZE, vr.LUT_STRETCH, vr.LUT_BYTES) == (rs.EQUALIZE, rs.STRETCH, 1024)


@pytest.mark.parametrize("tname", list(rs.TABLES))
@pytest.mark.parametrize("name", list(ps.BRUSHES))
def test_remap_apply_matches_the_numpy_restatement(base, name, tname):
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES[name]
    lut = rs.TABLES[tname]
    inside, _ = ps.spec_weights(base.shape[:3], centre, radius, 0)
    for strength in STRENGTHS:
        for op, _ in ps.OPS:
            for falloff, _ in ps.FALLOFFS:
                want = rs.spec_remap(base, lut, centre, radius, op, falloff, strength)
                got = vr.brush_remap_apply(brush(centre, radius, op, falloff, strength), lut, base.copy())
                assert_exact(got, want)
                for c in range(4):
                    if strength[c] == 0:
                        assert (want[..., c] == base[..., c]).all()
                assert (want[~inside] == base[~inside]).all()
                if name == "miss":
                    assert not inside.any() and (want == base).all()
                elif tname == "identity" and op == ps.SET:
                    assert (want == base).all()
                elif tname in ("perm", "invert") and not falloff:
                    assert (want[inside][:, 0] != base[inside][:, 0]).any()


def test_levels_over_the_whole_argument_space():
    """Every (in_lo, in_hi) pair for a handful of output pairs in both orders, on one channel mask each (every
    mask occurs); the channels outside the mask keep the bytes the table held.  The library is called through
    ctypes on one table that is reset by hand, so that the 228 480 calls stay quick."""
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    start = rs.TABLES["perm"]
    s = _lib.Lut()
    view = np.frombuffer(s, np.uint8).reshape(4, 256)
    checked = 0
    for in_lo in range(255):
        for in_hi in range(in_lo + 1, 256):
            for k, (out_lo, out_hi) in enumerate(OUT_PAIRS):
                mask = (in_hi + 5 * k + in_lo) % 16
                view[:] = start
                assert lib.vr_lut_levels(ctypes.byref(s), mask, in_lo, in_hi, out_lo, out_hi) == 0
                want = rs.spec_levels(start, mask, in_lo, in_hi, out_lo, out_hi)
                if not np.array_equal(view, want):
                    assert_exact(view.copy(), want)
                checked += 1
    assert checked == 255 * 256 // 2 * len(OUT_PAIRS)


def test_levels_round_halves_up_also_below_zero():
    """A falling line puts negative numerators under the floor: truncation towards zero would give other bytes."""
    ident = rs.spec_identity()
    falling = rs.spec_levels(ident, 1, 0, 4, 3, 0)[0][:5].tolist()     # 3 - 3 v / 4 at v = 0..4: 3, 2.25, 1.5, 0.75, 0
    assert falling == [3, 2, 2, 1, 0]
    v, den = np.arange(1, 4), 4
    truncated = 3 + np.trunc((2 * v * -3 + den) / (2 * den)).astype(int)
    assert truncated.tolist() != falling[1:4]
    import volumetricrenderer_amd as vr
    assert vr.lut_levels(0, 4, 3, 0, 1)[0][:5].tolist() == falling


def test_compose_and_aliasing():
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd import _lib
    T = rs.TABLES
    for a, b in (("perm", "invert"), ("invert", "perm"), ("levels_narrow", "posterise"), ("perm", "perm"), ("eq", "stretch")):
        want = rs.spec_compose(T[a], T[b])
        assert_exact(vr.lut_compose(T[a], T[b]), want)
        # out aliasing first, then, and (a == b) both
        for alias in (0, 1):
            sa, sb = _lib.Lut(), _lib.Lut()
            ctypes.memmove(ctypes.byref(sa), T[a].ctypes.data, 1024)
            ctypes.memmove(ctypes.byref(sb), T[b].ctypes.data, 1024)
            out = (sa, sb)[alias]
            _lib.call("vr_lut_compose", ctypes.byref(sa), ctypes.byref(sb), ctypes.byref(out))
            assert_exact(np.frombuffer(bytes(out), np.uint8).reshape(4, 256), want)
        if a == b:
            s = _lib.Lut()
            ctypes.memmove(ctypes.byref(s), T[a].ctypes.data, 1024)
            _lib.call("vr_lut_compose", ctypes.byref(s), ctypes.byref(s), ctypes.byref(s))
            assert_exact(np.frombuffer(bytes(s), np.uint8).reshape(4, 256), want)
    assert (rs.spec_compose(T["perm"], T["invert"]) != rs.spec_compose(T["invert"], T["perm"])).any()
    assert_exact(vr.lut_compose(T["invert"], T["invert"]), T["identity"])


def stats_cases(skewed):
    zero = np.zeros((4, 256), np.int64)
    one = zero.copy()
    one[:, 93] = 1234
    two = zero.copy()
    two[0, [3, 200]] = (5, 9)
    two[1, [0, 255]] = (1, 1)
    two[2, [100, 101]] = (2**31 - 1, 1)
    two[3, [17, 18]] = (1, 2**31 - 1)
    big = zero.copy()
    rng = np.random.default_rng(31)
    big[0, 40:200] = 2**31 - 1
    big[1, ::7] = rng.integers(1, 2**31, size=len(big[1, ::7]))
    big[2] = rng.integers(0, 2**31, size=256)
    big[2, 255] = 2**31 - 1
    big[3, [0, 128, 255]] = (2**31 - 1, 1, 2**31 - 1)
    real = rs.spec_hist(skewed, *ps.BRUSHES["interior"])
    real_whole = rs.spec_hist(skewed, *ps.BRUSHES["whole"], strength=(255, 128, 0, 1))
    return {"zero": zero, "one": one, "two": two, "big": big, "real": real, "real_whole": real_whole}


def test_stats_lut(skewed):
    import volumetricrenderer_amd as vr
    ident = rs.spec_identity()
    cases = stats_cases(skewed)
    for name, hist in cases.items():
        for kind in (rs.EQUALIZE, rs.STRETCH):
            for mask in (0, 5, 10, 15):
                want = rs.spec_stats_lut(hist, kind, mask)
                assert_exact(vr.stats_lut(host_stats(hist), kind, mask), want)
                for c in range(4):
                    if not mask >> c & 1:
                        assert (want[c] == ident[c]).all()
    for kind in (rs.EQUALIZE, rs.STRETCH):
        assert (rs.spec_stats_lut(cases["zero"], kind, 15) == ident).all()
        assert (rs.spec_stats_lut(cases["one"], kind, 15) == ident).all()
        two = rs.spec_stats_lut(cases["two"], kind, 15).astype(np.int64)
        for c, (lo, hi) in enumerate(((3, 200), (0, 255), (100, 101), (17, 18))):
            assert two[c][lo] == 0 and two[c][hi] == 255 and (two[c][:lo] == 0).all() and (two[c][hi:] == 255).all()
    # equalising two bins puts everything between them at 0, stretching spreads them
    assert (rs.spec_stats_lut(cases["two"], rs.EQUALIZE, 1)[0][3:200] == 0).all()
    assert rs.spec_stats_lut(cases["two"], rs.STRETCH, 1)[0][100] == ((100 - 3) * 255 + 98) // 197
    # only hist is read
    st = host_stats(cases["real"])
    other = vr.Stats(7, 9, np.array([1, 2, 3, 4], np.uint64), st.hist)
    assert_exact(vr.stats_lut(other, rs.EQUALIZE), vr.stats_lut(st, rs.EQUALIZE))


def test_invert_twice_and_identity(base):
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES["whole"]
    b = brush(centre, radius, ps.SET, 0, rs.FULL)
    once = vr.brush_remap_apply(b, rs.TABLES["invert"], base.copy())
    inside, _ = ps.spec_weights(base.shape[:3], centre, radius, 0)
    assert (once[inside] == 255 - base[inside]).all()
    assert_exact(vr.brush_remap_apply(b, rs.TABLES["invert"], once.copy()), base)
    for falloff in (0, 1):
        for strength in STRENGTHS:
            bb = brush(centre, radius, ps.SET, falloff, strength)
            assert_exact(vr.brush_remap_apply(bb, vr.lut_identity(), base.copy()), base)
    for op in (ps.ADD, ps.SUB):
        assert (vr.brush_remap_apply(brush(centre, radius, op, 0, rs.FULL), vr.lut_identity(), base.copy()) != base).any()


def test_refusals(base):
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd import _lib
    lut = rs.TABLES["perm"]
    vol = base.copy()
    good = brush((17, 11, 23), (3, 2, 4))
    bads = []
    for field, value in (("op", 3), ("op", -1), ("falloff", 2)):
        b = brush((17, 11, 23), (3, 2, 4))
        setattr(b, field, value)
        bads.append(b)
    for k, value in ((0, 256), (1, -1)):
        b = brush((17, 11, 23), (3, 2, 4))
        b.radius[k] = value
        bads.append(b)
    for k in range(2):
        b = brush((17, 11, 23), (3, 2, 4))
        b.reserved[k] = 1
        bads.append(b)
    for b in bads:
        with pytest.raises(vr.VRError) as e:
            vr.brush_remap_apply(b, lut, vol)
        assert e.value.status == 1 and "vr_brush_remap_apply" in str(e.value)
        assert (vol == base).all()
    s = _lib.Lut()
    ctypes.memmove(ctypes.byref(s), lut.ctypes.data, 1024)
    ptr = vol.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, ctypes.byref(s), ptr, ps.NX, ps.NY, ps.NZ), (ctypes.byref(good), None, ptr, ps.NX, ps.NY, ps.NZ),
                 (ctypes.byref(good), ctypes.byref(s), None, ps.NX, ps.NY, ps.NZ),
                 (ctypes.byref(good), ctypes.byref(s), ptr, 0, ps.NY, ps.NZ), (ctypes.byref(good), ctypes.byref(s), ptr, ps.NX, -1, ps.NZ),
                 (ctypes.byref(good), ctypes.byref(s), ptr, ps.NX, ps.NY, -2**31)):
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_brush_remap_apply", *args)
        assert e.value.status == 1
        assert (vol == base).all()
    with pytest.raises(ValueError):
        vr.brush_remap_apply(good, lut[:3], vol)
    with pytest.raises(ValueError):
        vr.brush_remap_apply(good, lut.astype(np.int32), vol)

    # the builders: *out stays as it was
    def out_unchanged(fn, *args):
        out = _lib.Lut()
        ctypes.memmove(ctypes.byref(out), lut.ctypes.data, 1024)
        with pytest.raises(vr.VRError) as e:
            _lib.call(fn, *[ctypes.byref(out) if a == "out" else a for a in args])
        assert e.value.status == 1 and fn in str(e.value)
        assert bytes(out) == lut.tobytes()

    for levels in ((-1, 5, 0, 255), (5, 5, 0, 255), (6, 5, 0, 255), (0, 256, 0, 255), (0, 255, -1, 255), (0, 255, 0, 256),
                   (0, 255, 256, 0), (2**31 - 1, -2**31, 0, 0)):
        out_unchanged("vr_lut_levels", "out", 15, *levels)
    for mask in (-1, 16, 2**31 - 1):
        out_unchanged("vr_lut_levels", "out", mask, 0, 255, 255, 0)
    st = _lib.VolumeStats()
    st.hist[0][3] = 5
    st.hist[0][9] = 5
    for kind, mask in ((2, 15), (-1, 15), (0, 16), (1, -1)):
        out_unchanged("vr_stats_lut", ctypes.byref(st), kind, mask, "out")
    out_unchanged("vr_stats_lut", None, 0, 15, "out")
    out_unchanged("vr_lut_compose", None, ctypes.byref(s), "out")
    out_unchanged("vr_lut_compose", ctypes.byref(s), None, "out")
    for fn, args in (("vr_lut_identity", (None,)), ("vr_lut_levels", (None, 15, 0, 255, 255, 0)),
                     ("vr_lut_compose", (ctypes.byref(s), ctypes.byref(s), None)), ("vr_stats_lut", (ctypes.byref(st), 0, 15, None))):
        with pytest.raises(vr.VRError) as e:
            _lib.call(fn, *args)
        assert e.value.status == 1 and "null" in str(e.value)
    # a mask of 0 is valid and changes nothing
    assert_exact(vr.lut_levels(0, 255, 255, 0, 0, lut), lut)


def test_prototypes_and_exports():
    from volumetricrenderer_amd import _lib
    src = open(os.path.join(ROOT, "include", "vr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for fn in ("vr_remap", "vr_remap_device", "vr_stats_lut_device", "vr_brush_remap_apply", "vr_lut_identity", "vr_lut_levels",
               "vr_lut_compose", "vr_stats_lut"):
        assert re.search(rf"\bvr_status\s+{fn}\s*\(", src), fn
        assert hasattr(lib, fn) and fn in _lib.exported_symbols()
    assert ctypes.sizeof(_lib.Lut) == 1024
    assert re.search(r"VR_LUT_EQUALIZE\s*=\s*0\s*,\s*VR_LUT_STRETCH\s*=\s*1", src)
    assert lib.vr_abi_version() == 2
