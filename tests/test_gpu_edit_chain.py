"""Edited volumes through the multi-frame march: one long-lived Renderer per (layout, variant) walks
the chain of tests/edit_chain.py -- one edit per member of the brush family on the 37 x 22 x 45 volume
-- and after EVERY edit, on the same context, everything below is exact (byte for byte):

  * get_volume() is the chained expected volume (the numpy restatements) and the returned box
    paint_spec.spec_box's;
  * "uniform_mask" is a subset of the channels that are uniform in the expected volume (the safety
    invariant) and, more strictly, equals edit_chain.expected_mask: kept while the edits leave the
    channel alone (b), kept after a SET at full strength wrote the uniform byte itself (c; vr.h
    vr_paint: "a result equal to what was there keeps it"), lost when an edit breaks it (d), and
    still lost after the last edit made it constant again (e; vr.h vr_update_volume).  The library
    exports no uniform value: a wrong one shows in the _u kernels' frames, which sample it;
  * kernel_variant names the layout's clamp kernel (no silent planar fallback) and the _u instance
    exactly while one channel is uniform and the early-out is off;
  * a plain render, render_group with four targets of one camera (under the option ladder
    quad_pairs 1, quad_pairs 0, quad_steps 0, quad_split 0), render_group with four cameras and
    render_pair with two equal the CPU oracle's frames of the expected volume, at early-out 0 and at
    edit_chain.EARLY (which ends rays on every step of a round, test_edit_chain_cpu.py);
  * the counters "quad_launches", "quad_split_launches", "quad_steps_launches" and
    "quad_pairs_launches" move as vr_internal.h's quad_instance and quad_split_layout predict for
    the current mask, early-out and layout -- restated in predict() from the expected mask, never
    read back from the library -- including the predicted 0 for the general instance of COL48 and
    BRICK4832 without early-out;
  * a grouped render issued twice with nothing changed (its first frame comes from the launch
    cache: "launch_cache_hits" moves) and once more straight after the NEXT edit, before anything
    else touches the context, shows that edit; so does the plain render after it.  With no uniform
    channel left an edit does not invalidate cached launches (vr_api.cpp box_edited), so that
    render is a cache hit too, and is asserted to be one.

At the end of a case the tally of counted launches shows that QUAD_PAIRS, QUAD_STEPS, QUAD_SPLIT and
QUAD_FRAMES each launched (COL48, BRICK4832; CORNERH has the plain QUAD instance only), for a
variant with a uniform channel both as that channel's _u instance and as the general one.

The frame is 70 x 37 RGBA8_UNORM (quads fall off the right and the bottom edge), max_steps 16,
step_scale 1, targets pre-filled with 0xA5, options as test_gpu_quad_pairs.setup.  The last test
takes the native frame loop (RcclBandPipeline, one rank, frame_group 4): four frames of one camera,
a paint, four more; the last frame is the oracle's of the painted volume.
"""
import os
import sys
from collections import Counter

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_chain as ec  # noqa: E402
import paint_spec as ps  # noqa: E402
from quad_cases import (BRICK4832, COL48, CORNERH, LADDER, MODES, SPLIT_LAYOUTS, counters, predict, refill,  # noqa: E402
                        set_options as setup)
import quad_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd.distributed import RcclBandPipeline

W, H, FMT = ec.W, ec.H, ec.FMT
NAMES = {COL48: "col48", BRICK4832: "brick4832", CORNERH: "cornerh"}
CASES = [(lay, v) for lay in SPLIT_LAYOUTS for v in ec.VARIANTS] + [(CORNERH, None), (CORNERH, 1)]
CASE_IDS = [f"{NAMES[lay]}-{ec.VARIANT_IDS[ec.VARIANTS.index(v)]}" for lay, v in CASES]
EARLIES = (0.0, ec.EARLY)


def end_early(variant, k):
    """The march a step leaves the context with (and the next edit's first renders run under): early-out 0 while a
    channel is uniform -- the _u instance is then the cached launch that has to go -- else alternating."""
    return 0.0 if ec.expected_mask(variant, k) or k % 2 == 0 else ec.EARLY


def target(rr):
    return qc.target(rr, (W, H), FMT)


def same(got, want, what):
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    assert g.shape == want.shape, what
    bad = np.argwhere(g != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ from the oracle's frame, first (y, x, c) {bad[:4].tolist()}"


@pytest.mark.parametrize("layout,variant", CASES, ids=CASE_IDS)
def test_every_render_call_after_every_edit(oracle, layout, variant):
    edits, vols = ec.expected(variant)
    cams = [ec.shader_data(i) for i in range(4)]
    marches = {e: ec.march_params(e) for e in EARLIES}
    name = NAMES[layout]
    tally = Counter()

    def ref(k, cam, early):
        return ec.oracle_frame(oracle, vols[k], cam, early)

    with vr.Renderer(0) as r:
        setup(r, layout)
        r.set_volume(vols[0])
        held = [target(r) for _ in range(4)]      # the grouped render that is repeated, and issued again after the next edit
        outs = [target(r) for _ in range(4)]      # every other render
        for k in range(len(vols)):
            e = edits[k - 1] if k else None
            at = f"{name}, step {k} " + (f"{e.name} ({e.brush}){' (' + e.phase + ')' if e.phase else ''}" if e else "install")
            want_mask = ec.expected_mask(variant, k)
            if e:
                # ---- the edit, then the held grouped render and a plain one before anything else touches the context
                before_mask, early = ec.expected_mask(variant, k - 1), end_early(variant, k - 1)
                hits = r.get_option("launch_cache_hits")
                assert e.run(r, vr, torch) == e.returns, f"{at}: the returned box"
                refill(held)
                r.render_group(W, H, FMT, held, cameras=None)
                for i in range(4):
                    same(held[i], ref(k, 0, early), f"{at}: render_group straight after the edit, frame {i}")
                refill(held[:1])
                r.render(W, H, FMT, out=held[0])
                same(held[0], ref(k, 0, early), f"{at}: render straight after the edit")
                # a uniform channel: the edit re-armed the read-back, nothing cached is used; none: cached launches stay
                assert r.get_option("launch_cache_hits") - hits == (0 if before_mask else 2), f"{at}: launch cache hits"
            # ---- the volume and the uniform channels
            got = r.get_volume()
            bad = np.argwhere(got != vols[k])
            assert bad.size == 0, f"{at}: get_volume differs at {len(bad)} bytes, first (z, y, x, c) {bad[:4].tolist()}"
            mask = r.get_option("uniform_mask")
            assert mask & ~ec.truly_uniform(vols[k]) == 0, f"{at}: uniform_mask {mask} names a channel that is not uniform"
            assert mask == want_mask, f"{at}: uniform_mask {mask}, expected {want_mask}"
            # ---- every render call, without and with the early-out
            for early in EARLIES:
                r.set_march(marches[early])
                r.set_shader_data(*cams[0])
                variant_name = r.kernel_variant
                u_kernel = not early and want_mask in (1, 2, 4, 8)
                assert variant_name.startswith(f"grid_{name}_clamp"), f"{at}: kernel_variant {variant_name}"
                assert variant_name.endswith("_u" + "RGBA"[variant or 0]) == u_kernel and ("_u" in variant_name) == u_kernel, \
                    f"{at}, early-out {early}: kernel_variant {variant_name}"
                what = f"{at}, early-out {early}"
                refill(outs[:1])
                r.render(W, H, FMT, out=outs[0])
                same(outs[0], ref(k, 0, early), f"{what}: render")
                for split, steps, pairs in LADDER:
                    for opt, v in (("quad_split", split), ("quad_steps", steps), ("quad_pairs", pairs)):
                        r.set_option(opt, v)
                    refill(outs)
                    c0 = counters(r)
                    r.render_group(W, H, FMT, outs, cameras=[cams[0]] * 4)
                    torch.cuda.synchronize()
                    moved = tuple(b - a for a, b in zip(c0, counters(r)))
                    opts = f"quad_split {split}, quad_steps {steps}, quad_pairs {pairs}"
                    assert moved == predict(layout, early, want_mask, split, steps, pairs), \
                        f"{what}, {opts}: (QUAD, split, step-round, paired) launches {moved}"
                    for i in range(4):
                        same(outs[i], ref(k, 0, early), f"{what}: render_group of one camera, {opts}, frame {i}")
                    tally[MODES[moved], "u" if u_kernel else "general"] += 1
                for opt in ("quad_split", "quad_steps", "quad_pairs"):
                    r.set_option(opt, 1)
                refill(outs)
                g0, p0, c0 = r.get_option("group_launches"), r.get_option("pair_launches"), counters(r)
                r.render_group(W, H, FMT, outs, cameras=cams)
                for i in range(4):
                    same(outs[i], ref(k, i, early), f"{what}: render_group of four cameras, frame {i}")
                refill(outs[:2])
                r.render_pair(W, H, FMT, outs[0], outs[1], cameras=cams[1:3])
                for i in range(2):
                    same(outs[i], ref(k, 1 + i, early), f"{what}: render_pair, frame {i}")
                assert (r.get_option("group_launches") - g0, r.get_option("pair_launches") - p0) == (1, 3), what
                assert counters(r) == c0, f"{what}: a QUAD launch for frames of different cameras"
            # ---- the held grouped render, twice with nothing changed: its first frame is planned once and then cached
            early = end_early(variant, k)
            r.set_march(marches[early])
            r.set_shader_data(*cams[0])
            for _ in range(2):   # (the second is planned after the first one's region lists have settled, and cached)
                refill(held[:1])
                r.render(W, H, FMT, out=held[0])
                same(held[0], ref(k, 0, early), f"{at}: render into the held target")
            for n in range(2):
                hits = r.get_option("launch_cache_hits")
                refill(held)
                r.render_group(W, H, FMT, held, cameras=None)
                for i in range(4):
                    same(held[i], ref(k, 0, early), f"{at}: held render_group {n}, frame {i}")
                assert r.get_option("launch_cache_hits") - hits == 1, f"{at}: held render_group {n} missed the launch cache"
        # ---- what really launched in this case
        print(f"{name}, {ec.VARIANT_IDS[ec.VARIANTS.index(variant)]}: counted launches {dict(tally)}")
        modes = ("QUAD_PAIRS", "QUAD_STEPS", "QUAD_SPLIT", "QUAD_FRAMES") if layout in SPLIT_LAYOUTS else ("QUAD_FRAMES",)
        for mode in modes:
            assert tally[mode, "general"] > 0, f"{name}: no {mode} launch of the general instance; {dict(tally)}"
            if variant is not None:
                assert tally[mode, "u"] > 0, f"{name}: no {mode} launch of the _u{'RGBA'[variant]} instance; {dict(tally)}"
        if layout in SPLIT_LAYOUTS:
            assert tally["QUAD_NONE", "general"] > 0    # the general instance without early-out: the predicted 0
        else:
            assert set(m for m, _ in tally) == {"QUAD_FRAMES"}


@pytest.mark.parametrize("pairing", [1, 2])
@pytest.mark.parametrize("variant,early", [(1, 0.0), (None, ec.EARLY)], ids=["uG", "general_early_out"])
def test_native_frame_loop_shows_the_paint(oracle, variant, early, pairing):
    """Four frames of one camera through the loop's four-frame arm, a paint that leaves the uniform channel alone,
    four more: the last frame is the oracle's of the painted volume, and both groups were QUAD launches."""
    vol = ec.base(variant)
    centre, radius = ec.BRUSHES["wide"]
    strength = tuple(0 if c == ec.quiet(variant) else 255 for c in range(4))
    painted = ps.spec_apply(vol, centre, radius, ps.SET, 1, ps.VALUE, strength)
    assert (ec.oracle_frame(oracle, vol, 0, early) != ec.oracle_frame(oracle, painted, 0, early)).any()
    with vr.Renderer(0) as r:
        setup(r, COL48)
        r.set_volume(vol)
        r.set_march(ec.march_params(early))
        r.set_shader_data(*ec.shader_data(0))
        pl = RcclBandPipeline(r, W, H, FMT, band_rows=16, world=1, rank=0)
        try:
            pl.pairing = pairing
            pl.frame_group = 4
            g0, c0 = r.get_option("group_launches"), counters(r)
            pl.run_frames(4)
            same(pl.frame(), ec.oracle_frame(oracle, vol, 0, early), "the fourth frame")
            assert r.paint(centre, radius, ps.SET, 1, ps.VALUE, strength) == ps.spec_box(centre, radius)
            pl.run_frames(4)
            same(pl.frame(), ec.oracle_frame(oracle, painted, 0, early), "the fourth frame after the paint")
            assert np.array_equal(r.get_volume(), painted)
            mask = 0 if variant is None else 1 << variant
            assert r.get_option("uniform_mask") == mask
            assert r.get_option("group_launches") - g0 == 2
            want = predict(COL48, early, mask, 1, 1, 1)
            assert want == (1, 1, 1, 1)
            assert tuple(b - a for a, b in zip(c0, counters(r))) == tuple(2 * w for w in want)
        finally:
            pl.close()
