"""The conditions of the state-transition harness (tests/transitions.py,
test_gpu_transitions.py), checked against the oracle alone so that they hold
before any kernel runs: the base frames are not empty, no mutation that is
meant to change pixels is a no-op, the serpentine sets of the sort-reuse bug
collide in size and differ in content, and the Python row mapping is the
library's."""
import numpy as np
import pytest

import transitions as T


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("name", sorted(T.ALL_BASES))
def test_base_frames_cover_the_target(oracle, name):
    """Every base frame covers at least 20 % of its pixels (0.43 for the
    camera reference_shader_data(96/112, 20, 15)), its selected rows hold
    covered pixels with a non-zero value, and steps are executed there."""
    b = T.ALL_BASES[name]
    assert T.coverage(oracle, b) >= 0.20
    rows, px, steps = T.expected(oracle, b)
    assert steps > 0
    assert (px[..., 0] > 0).mean() >= 0.10


# mutations that leave the selected rows' expected pixels as they are, by name
NO_PIXEL_CHANGE = {"inplace", "pad3", "otherbuf",
                   "wedges3", "supertile1", "split2", "region_order0", "tpw1", "uniform_skip0", "empty_fill0",
                   "region_gpu0", "schedule0", "schedule4", "wg_waves8", "wg_waves16",
                   "layout0", "layout1", "layout12", "layout14", "layout15",
                   "lattice0", "count1", "shadow_defer0", "shadow_cache1", "sort_reuse31"}


@pytest.mark.parametrize("base,mutation", T.CASES, ids=T.CASE_IDS)
def test_mutation_is_not_a_no_op(oracle, base, mutation):
    """expected(B) != expected(B + M) for every mutation meant to change
    pixels; the others are listed in NO_PIXEL_CHANGE, change the scene record
    all the same, and leave the expected pixels equal."""
    b = T.ALL_BASES[base]
    s = mutation(b)
    assert s != b and T.target_valid(s.target) and T.target_valid(b.target)
    rows0, px0, steps0 = T.expected(oracle, b)
    rows1, px1, steps1 = T.expected(oracle, s)
    assert mutation.pixels == (mutation.name not in NO_PIXEL_CHANGE)
    if mutation.pixels:
        assert not _same(px0, px1)
    else:
        assert _same(px0, px1) and np.array_equal(np.sort(rows0), np.sort(rows1))
        if mutation.name == "count1" and dict(b.proc or ()).get("shadow_steps", 0) > 0:
            assert steps1 > steps0   # the shadow samples are counted
        else:
            assert steps1 == steps0
    if mutation.name == "early0.3":
        assert steps1 < 0.95 * steps0   # rays do end early on the dense bases


def test_flip_sets_collide_in_size_and_differ():
    t0 = T.Target()
    t2 = T.Target(band_flip=2)
    r0, r2 = T.target_rows(t0), T.target_rows(t2)
    assert len(r0) == len(r2) == 48
    assert sorted(set(r0 // 16)) == [0, 3, 6] and sorted(set(r2 // 16)) == [0, 5, 6]
    rr = T.target_rows(T.Target(mode="range", band_rows=48, band_stride=1, band_first=16))
    assert len(rr) == 48 and rr[0] == 16 and rr[-1] == 63


@pytest.mark.parametrize("base", ["G0", "P", "PS"])
def test_flip_sets_expected_images_differ(oracle, base):
    """The sets (16, 3, 0) with flip 0 and flip 2 pack 48 rows each (bands 0,
    3, 6 and 0, 5, 6) and their expected images differ widely: band 3 and band
    5 cover different pixel counts."""
    b = T.BASES[base]
    f = T.Mutation("flip2", "target", (("band_flip", 2),))(b)
    _, px0, s0 = T.expected(oracle, b)
    _, px2, s2 = T.expected(oracle, f)
    assert px0.shape == px2.shape
    assert (px0[16:32, :, 0] > 0).sum() != (px2[16:32, :, 0] > 0).sum()
    assert (px0 != px2).sum() > 500 and s0 != s2


def _all_targets():
    ts = {T.ALL_BASES[b].target for b in T.ALL_BASES}
    ts |= {m(T.ALL_BASES[b]).target for b, m in T.CASES}
    for fam in T.WALKS:
        ts |= {s.target for s in T.walk(fam)[1]}
    return sorted(ts, key=repr)


def test_row_mapping_agrees_with_the_library():
    """len(target_rows) is vr_band_rows_packed for every target of the single
    walks and the random walks (band sets, whole frames; a row range packs
    its rows cut at the frame), the selected rows are distinct, lie inside the
    frame, and only a last band runs past it."""
    from volumetricrenderer_amd import _lib
    packed = _lib.load().vr_band_rows_packed
    ts = _all_targets()
    assert len(ts) > 30
    for t in ts:
        assert T.target_valid(t), t
        rows = T.target_rows(t)
        if t.mode == "range":
            assert len(rows) == max(0, min(t.band_rows, t.H - t.band_first)), t
        else:
            assert len(rows) == packed(t.H, t.band_rows, t.band_stride, t.band_first, t.band_flip), t
        sel = rows[rows >= 0]
        assert len(set(sel)) == len(sel) and sel.max() < t.H and (np.diff(sel) > 0).all(), t
        past = np.nonzero(rows < 0)[0]
        assert past.size == 0 or (past.min() >= len(rows) - t.band_rows and len(sel) + past.size == len(rows)), t


def test_walks_are_deterministic_and_single_steps():
    """Each family's walk is the same on every machine, every scene differs
    from the one before it and is a valid target for the default build."""
    for fam in T.WALKS:
        base, a = T.walk(fam)
        assert a == T.walk(fam)[1] and len(a) == T.WALK_STEPS
        prev = base
        for s in a:
            assert s != prev and T.target_valid(s.target) and not T.needs_experiments(s)
            assert (s.proc is None) == (base.proc is None)
            prev = s
        assert len(set(a)) > T.WALK_STEPS // 2


def test_strip_counts_agree_with_step_counts(oracle):
    """The two ways expected() counts steps agree where both apply: the
    oracle's own 8-row band renders sum what oracle.step_counts gives per row
    when no ray ends early."""
    for name in ("G0", "PS"):
        b = T.BASES[name]
        _, steps = T.oracle_frame(oracle, b)
        s2, evals = T.oracle_strips(oracle, b)
        assert np.array_equal(steps, s2)
        assert evals is None or (evals >= s2).all() and evals.sum() > s2.sum()
