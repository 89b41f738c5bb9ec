"""The native frame loop with pairing (the context option "frame_pairing"): a one-rank
pipeline takes its frames two at a time through vr_render_pair.  200 x 120,
32 steps, cameras given; every frame compared byte for byte with a plain
render of its camera."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd.distributed import RcclBandPipeline

W, H, STEPS = 200, 120, 32
FMT = 1   # RGBA8_UNORM


@pytest.fixture(scope="module")
def scene():
    """(renderer, cameras, plain renders of the cameras), made once."""
    vol = np.random.default_rng(77).integers(0, 256, size=(64, 64, 64, 4), dtype=np.uint8)
    with vr.Renderer(0) as r:
        r.set_layout_preference(15)   # COL48: the paired kernel of the flagship layout
        r.set_option("split", 1)      # one lane per ray (a frame this small would auto-split, which is not paired)
        r.set_volume(vol)
        r.set_march(vr.march_defaults(max_steps=STEPS))
        cams = [vr.reference_shader_data(W / H, 1.6 * i, 15.0) for i in range(7)]
        refs = []
        for c in cams:
            r.set_shader_data(*c)
            refs.append(r.render(W, H, FMT).cpu().numpy())
        yield r, cams, refs


@pytest.fixture(scope="module")
def pipe(scene):
    r = scene[0]
    pl = RcclBandPipeline(r, W, H, FMT, band_rows=16, world=1, rank=0)
    yield pl
    pl.close()


def frame_of(pl):
    got = pl.frame().cpu().numpy()
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("pairing", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_last_frame_is_its_camera(scene, pipe, pairing, n):
    r, cams, refs = scene
    pipe.pairing = pairing
    assert pipe.pairing == pairing
    n0 = r.get_option("pair_launches")
    pipe.run_frames(n, cameras=cams[:n])
    assert np.array_equal(frame_of(pipe), refs[n - 1])
    assert r.get_option("pair_launches") - n0 == (n // 2 if pairing else 0)


@pytest.mark.parametrize("pairing", [1, 2])
def test_parity_carries_over_between_runs(scene, pipe, pairing):
    r, cams, refs = scene
    pipe.pairing = pairing
    pipe.run_frames(4, cameras=cams[:4])
    assert np.array_equal(frame_of(pipe), refs[3])
    pipe.run_frames(3, cameras=cams[4:7])
    assert np.array_equal(frame_of(pipe), refs[6])
    pipe.run_frames(2, cameras=cams[1:3])
    assert np.array_equal(frame_of(pipe), refs[2])


@pytest.mark.parametrize("pairing", [1, 2])
def test_static_camera_renders_every_frame(scene, pipe, pairing):
    """No cameras given: both frames of a pair are rendered with the current shader data."""
    r, cams, refs = scene
    pipe.pairing = pairing
    r.set_shader_data(*cams[5])
    pipe.run_frames(4)
    assert np.array_equal(frame_of(pipe), refs[5])


@pytest.mark.parametrize("pairing", [1, 2])
def test_sampled_pairs(scene, pipe, pairing):
    r, cams, refs = scene
    pipe.pairing = pairing
    ms = pipe.run_frames(5, cameras=cams[:5], sample_every=1)
    assert math.isfinite(ms) and ms > 0.0
    busy, span = pipe.sampled_busy()
    assert 0.0 < busy <= span + 1e-6
    assert np.array_equal(frame_of(pipe), refs[4])


def test_loopback_ranks_ignore_pairing():
    """Two ranks in one process (test_native_pipeline_loopback_ranks' 500 x 283 geometry): the
    multi-rank path keeps one launch per frame whatever the switch says."""
    Wl, Hl = 500, 283
    with vr.Renderer(0) as r:
        r.generate_volume(vr.volume_recipe_defaults(size=64))
        r.set_shader_data(*vr.reference_shader_data(Wl / Hl, -30.0, 40.0))
        r.set_march(vr.march_defaults())
        full = r.render(Wl, Hl, FMT).cpu().numpy()
        pl = RcclBandPipeline(r, Wl, Hl, FMT, band_rows=16, world=2, rank=0, loopback=True, render_streams=2)
        try:
            pl.pairing = 1
            n0 = r.get_option("pair_launches")
            pl.run_frames(3)
            pl.barrier()
            assert np.array_equal(pl.frame().cpu().numpy(), full)
            assert r.get_option("pair_launches") == n0
        finally:
            pl.close()
