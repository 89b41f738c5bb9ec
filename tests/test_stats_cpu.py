"""The statistics under a brush, the checks that need no GPU: vr_brush_stats_host
and vr_box_stats_host against the numpy restatement (tests/stats_spec.py) on
every brush of paint_spec.BRUSHES x falloff x two strength sets and on boxes
with every channel mask; the conditions those inputs must meet; edge volumes;
vr_stats_summary against numpy on the byte lists; refusals that leave the out
struct as it was; prototypes and exports.  Everything is exact."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paint_spec as ps  # noqa: E402
from brush_harness import base  # noqa: E402,F401
import stats_spec as ss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"vr_brush_stats": 4, "vr_box_stats": 10, "vr_brush_stats_host": 6, "vr_box_stats_host": 12, "vr_stats_summary": 2}


def brush(centre, radius, falloff=0, strength=ss.FULL, op=0, value=(1, 2, 3, 4)):
    import volumetricrenderer_amd as vr
    return vr.make_brush(centre, radius, op, falloff, value, strength)


@pytest.mark.parametrize("strength", ss.STRENGTHS, ids=["rgb", "a"])
@pytest.mark.parametrize("falloff,fname", ps.FALLOFFS, ids=[n for _, n in ps.FALLOFFS])
@pytest.mark.parametrize("name", list(ps.BRUSHES))
def test_brush_stats_host_matches_the_numpy_restatement(base, name, falloff, fname, strength):
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES[name]
    want = ss.spec_brush_stats(base, centre, radius, falloff, strength)
    got = vr.brush_stats_host(brush(centre, radius, falloff, strength), base)
    ss.assert_stats(got, want, name)
    # op and value are validated and then ignored
    ss.assert_stats(vr.brush_stats_host(brush(centre, radius, falloff, strength, op=2, value=(9, 9, 9, 9)), base), want, name)
    # the conditions on the inputs: a weaker input must not hide a failure
    if name == "miss":
        assert got.count == 0 and got.weight == 0 and not got.wsum.any() and not got.hist.any()
        return
    assert got.count > 0
    if falloff and name != "texel":
        assert got.weight < 256 * got.count
    else:
        assert got.weight == 256 * got.count
    for c in range(4):
        if strength[c]:
            assert int(got.hist[c].sum()) == got.count
        else:
            assert not got.hist[c].any() and got.wsum[c] == 0
    assert any(strength) and any(s == 0 for s in strength)


def test_no_channel_selected_still_counts(base):
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES["interior"]
    got = vr.brush_stats_host(brush(centre, radius, 1, (0, 0, 0, 0)), base)
    want = ss.spec_brush_stats(base, centre, radius, 1, (0, 0, 0, 0))
    ss.assert_stats(got, want)
    assert got.count > 0 and got.weight > 0 and not got.hist.any() and not got.wsum.any()


@pytest.mark.parametrize("mask", range(16))
def test_box_stats_host(base, mask):
    import volumetricrenderer_amd as vr
    for origin, extent in (((0, 0, 0), (ps.NX, ps.NY, ps.NZ)), ((36, 21, 44), (1, 1, 1)), ((5, 0, 7), (1, 22, 3))):
        got = vr.box_stats_host(base, origin, extent, mask)
        ss.assert_stats(got, ss.spec_box_stats(base, origin, extent, mask), (origin, extent))
        n = extent[0] * extent[1] * extent[2]
        assert got.count == n and got.weight == 256 * n
        for c in range(4):
            assert int(got.hist[c].sum()) == (n if mask >> c & 1 else 0)


def test_edge_volumes():
    import volumetricrenderer_amd as vr
    one = np.array([[[[9, 200, 0, 255]]]], np.uint8)
    for falloff in (0, 1):
        for radius in ((0, 0, 0), (255, 255, 255)):
            got = vr.brush_stats_host(brush((0, 0, 0), radius, falloff), one)
            ss.assert_stats(got, ss.spec_brush_stats(one, (0, 0, 0), radius, falloff, ss.FULL))
            assert got.count == 1 and got.weight == 256 and got.wsum.tolist() == [9 * 256, 200 * 256, 0, 255 * 256]
    ss.assert_stats(vr.box_stats_host(one, (0, 0, 0), (1, 1, 1), 0xF), ss.spec_box_stats(one, (0, 0, 0), (1, 1, 1), 0xF))
    thin = np.random.default_rng(11).integers(0, 256, size=(1, 3, 2, 4), dtype=np.uint8)   # 2 x 3 x 1
    for falloff in (0, 1):
        for centre, radius in (((1, 1, 0), (4, 4, 4)), ((0, 2, 0), (1, 1, 0)), ((2**31 - 1, 1, 0), (255, 255, 255)),
                               ((-2**31, 1, 0), (255, 0, 255))):
            got = vr.brush_stats_host(brush(centre, radius, falloff, (255, 0, 7, 1)), thin)
            ss.assert_stats(got, ss.spec_brush_stats(thin, centre, radius, falloff, (255, 0, 7, 1)), (centre, radius))
    for mask in range(16):
        ss.assert_stats(vr.box_stats_host(thin, (0, 0, 0), (2, 3, 1), mask), ss.spec_box_stats(thin, (0, 0, 0), (2, 3, 1), mask))
        ss.assert_stats(vr.box_stats_host(thin, (1, 2, 0), (1, 1, 1), mask), ss.spec_box_stats(thin, (1, 2, 0), (1, 1, 1), mask))
    with pytest.raises(ValueError):
        vr.brush_stats_host(brush((0, 0, 0), (1, 1, 1)), np.zeros((2, 2, 2, 3), np.uint8))


def check_summary(st, got):
    want = ss.spec_summary(st)
    for k in ("n", "min", "max", "mean", "wmean", "median"):
        assert np.array_equal(getattr(got, k), want[k]), (k, getattr(got, k), want[k])


def test_stats_summary_against_numpy(base):
    import volumetricrenderer_amd as vr
    cases = []
    for name in ("interior", "texel", "straddle", "whole"):
        for falloff in (0, 1):
            for strength in ss.STRENGTHS + [ss.FULL]:
                cases.append(vr.brush_stats_host(brush(*ps.BRUSHES[name], falloff, strength), base))
    cases.append(vr.box_stats_host(base, (0, 0, 0), (ps.NX, ps.NY, ps.NZ), 0b0101))
    cases.append(vr.box_stats_host(base, (3, 4, 5), (2, 1, 1), 0xF))      # n = 2: the median is the lower byte
    skew = np.zeros((3, 3, 3, 4), np.uint8)
    skew[..., 0] = 255
    skew[0, 0, 0] = (0, 7, 254, 1)
    skew.reshape(-1, 4)[:14, 3] = 200                                       # 14 of 27: the median sits on the majority
    cases.append(vr.box_stats_host(skew, (0, 0, 0), (3, 3, 3), 0xF))
    cases.append(vr.brush_stats_host(brush((1, 1, 1), (1, 1, 1), 1), skew))
    seen_round_up = False
    for st in cases:
        got = vr.stats_summary(st)
        check_summary(dict(count=st.count, weight=st.weight, wsum=st.wsum.astype(np.int64), hist=st.hist.astype(np.int64)), got)
        for c in range(4):
            n = int(st.hist[c].sum())
            if n and (2 * int((np.arange(256) * st.hist[c].astype(np.int64)).sum())) % (2 * n) >= n:
                seen_round_up = True
    assert seen_round_up, "no case rounds its mean upwards"
    # n = 0: an empty result, and an unselected channel next to selected ones
    empty = vr.stats_summary(vr.brush_stats_host(brush(*ps.BRUSHES["miss"]), base))
    for k in empty._fields:
        assert not getattr(empty, k).any(), k
    part = vr.stats_summary(vr.box_stats_host(base, (0, 0, 0), (4, 4, 4), 0b0010))
    assert part.n.tolist() == [0, 64, 0, 0]
    for k in ("min", "max", "mean", "wmean", "median"):
        assert getattr(part, k)[[0, 2, 3]].tolist() == [0, 0, 0] and (k == "min" or getattr(part, k)[1] > 0)
    # the raw struct goes in as well
    from volumetricrenderer_amd import _lib
    raw = _lib.VolumeStats()
    b = brush(*ps.BRUSHES["interior"], 1)
    assert _lib.load().vr_brush_stats_host(ctypes.byref(b), base.ctypes.data_as(ctypes.c_void_p), ps.NX, ps.NY, ps.NZ,
                                           ctypes.byref(raw)) == 0
    check_summary(ss.spec_brush_stats(base, *ps.BRUSHES["interior"], 1, ss.FULL), vr.stats_summary(raw))


def test_refusals_leave_the_out_struct_untouched(base):
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    out = _lib.VolumeStats()
    ctypes.memset(ctypes.byref(out), 0xA5, ctypes.sizeof(out))
    keep = bytes(out)
    vp = base.ctypes.data_as(ctypes.c_void_p)
    dims = (ps.NX, ps.NY, ps.NZ)
    bad = [brush((1, 1, 1), (2, -1, 2)), brush((1, 1, 1), (256, 2, 2)), brush((1, 1, 1), (2, 2, 2), falloff=2),
           brush((1, 1, 1), (2, 2, 2), op=3), brush((1, 1, 1), (2, 2, 2), op=-1)]
    for k in range(2):
        b = brush((1, 1, 1), (2, 2, 2))
        b.reserved[k] = 1
        bad.append(b)
    for b in bad:
        assert lib.vr_brush_stats_host(ctypes.byref(b), vp, *dims, ctypes.byref(out)) == 1   # VR_ERR_INVALID
        assert "vr_brush_stats_host:" in lib.vr_last_error().decode()
        assert lib.vr_brush_stats(ctypes.c_void_p(8), ctypes.byref(b), ctypes.c_void_p(8), None) == 1
        assert bytes(out) == keep
    good = brush((1, 1, 1), (2, 2, 2))
    for d in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert lib.vr_brush_stats_host(ctypes.byref(good), vp, *d, ctypes.byref(out)) == 1
        assert lib.vr_box_stats_host(vp, *d, 0, 0, 0, 1, 1, 1, 15, ctypes.byref(out)) == 1
    for mask in (-1, 16, 255, 2**31 - 1):
        assert lib.vr_box_stats_host(vp, *dims, 0, 0, 0, 1, 1, 1, mask, ctypes.byref(out)) == 1
        assert "channel_mask" in lib.vr_last_error().decode()
        assert lib.vr_box_stats(ctypes.c_void_p(8), 0, 0, 0, 1, 1, 1, mask, ctypes.c_void_p(8), None) == 1
    for box in ((-1, 0, 0, 1, 1, 1), (0, 0, 0, ps.NX + 1, 1, 1), (36, 0, 0, 2, 1, 1), (0, 21, 0, 1, 2, 1), (0, 0, 45, 1, 1, 1),
                (0, 0, 0, 0, 1, 1), (0, 0, 0, 1, -1, 1), (2**31 - 1, 0, 0, 2**31 - 1, 1, 1)):
        assert lib.vr_box_stats_host(vp, *dims, *box, 15, ctypes.byref(out)) == 1, box
        assert "vr_box_stats_host:" in lib.vr_last_error().decode()
    assert bytes(out) == keep
    summ = _lib.StatsSummary()
    for name, args in (("vr_brush_stats_host", (None, vp, *dims, ctypes.byref(out))),
                       ("vr_brush_stats_host", (ctypes.byref(good), None, *dims, ctypes.byref(out))),
                       ("vr_brush_stats_host", (ctypes.byref(good), vp, *dims, None)),
                       ("vr_box_stats_host", (None, *dims, 0, 0, 0, 1, 1, 1, 15, ctypes.byref(out))),
                       ("vr_box_stats_host", (vp, *dims, 0, 0, 0, 1, 1, 1, 15, None)),
                       ("vr_stats_summary", (None, ctypes.byref(summ))),
                       ("vr_stats_summary", (ctypes.byref(out), None)),
                       ("vr_brush_stats", (None, ctypes.byref(good), ctypes.c_void_p(8), None)),
                       ("vr_brush_stats", (ctypes.c_void_p(8), None, ctypes.c_void_p(8), None)),
                       ("vr_brush_stats", (ctypes.c_void_p(8), ctypes.byref(good), None, None)),
                       ("vr_box_stats", (None, 0, 0, 0, 1, 1, 1, 15, ctypes.c_void_p(8), None)),
                       ("vr_box_stats", (ctypes.c_void_p(8), 0, 0, 0, 1, 1, 1, 15, None, None))):
        assert getattr(lib, name)(*args) == 1, name
        msg = lib.vr_last_error().decode()
        assert name + ":" in msg and "null" in msg, msg
    assert bytes(out) == keep
    # and a good call overwrites the struct
    assert lib.vr_brush_stats_host(ctypes.byref(brush(*ps.BRUSHES["miss"])), vp, *dims, ctypes.byref(out)) == 0
    assert bytes(out) == bytes(ctypes.sizeof(out))


def test_prototypes_exports_and_signatures():
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vr_[a-z_0-9]+)\s*\(", src))
    for name, nargs in NEW.items():
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
        m = re.search(r"vr_status\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib._SIGS[name][1]), name
        assert _lib._SIGS[name][0] is ctypes.c_int
    assert ctypes.sizeof(_lib.VolumeStats) == 8240 == vr.VOLUME_STATS_BYTES and _lib.VolumeStats.hist.offset == 48
    assert ctypes.sizeof(_lib.StatsSummary) == 112
    assert lib.vr_abi_version() == 2
    for fn in (vr.Renderer.brush_stats, vr.Renderer.box_stats, vr.brush_stats_host, vr.box_stats_host, vr.stats_summary,
               vr.unpack_stats):
        assert callable(fn)
    for name in ("brush_stats_host", "box_stats_host", "stats_summary", "VolumeStats", "StatsSummary"):
        assert name in vr.__all__, name
