"""The native frame loop with four frames per launch (the context option "frame_group" =
4 under "frame_pairing" 1 and 2): a one-rank pipeline takes its frames four at a time
through vr_render_group, the remainder as a pair and / or a single frame.  70 x 44, 32
steps, cameras given; every frame compared byte for byte with a plain render of its
camera through the last-frame rule (k frames run, frame() against camera k - 1)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd.distributed import RcclBandPipeline

W, H, STEPS = 70, 44, 32
FMT = 1   # RGBA8_UNORM


@pytest.fixture(scope="module")
def scene():
    """(renderer, cameras, plain renders of the cameras), made once."""
    vol = np.random.default_rng(78).integers(0, 256, size=(64, 64, 64, 4), dtype=np.uint8)
    with vr.Renderer(0) as r:
        r.set_layout_preference(15)   # COL48: the grouped kernel of the flagship layout
        r.set_option("split", 1)      # one lane per ray (a frame this small would auto-split, which is not grouped)
        r.set_volume(vol)
        r.set_march(vr.march_defaults(max_steps=STEPS))
        cams = [vr.reference_shader_data(W / H, 1.6 * i, 15.0) for i in range(9)]
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


def launches(r):
    return r.get_option("group_launches"), r.get_option("pair_launches")


@pytest.mark.parametrize("pairing", [1, 2])
@pytest.mark.parametrize("n", range(1, 10))
def test_last_frame_is_its_camera(scene, pipe, pairing, n):
    r, cams, refs = scene
    pipe.pairing = pairing
    pipe.frame_group = 4
    assert pipe.frame_group == 4
    g0, p0 = launches(r)
    pipe.run_frames(n, cameras=cams[:n])
    assert np.array_equal(frame_of(pipe), refs[n - 1])
    g1, p1 = launches(r)
    assert g1 - g0 == n // 4 and p1 - p0 == n // 2   # (pair_launches: two per four-frame launch)


@pytest.mark.parametrize("pairing", [1, 2])
def test_parity_carries_over_between_runs(scene, pipe, pairing):
    r, cams, refs = scene
    pipe.pairing = pairing
    pipe.frame_group = 4
    pipe.run_frames(4, cameras=cams[:4])
    assert np.array_equal(frame_of(pipe), refs[3])
    pipe.run_frames(5, cameras=cams[4:9])
    assert np.array_equal(frame_of(pipe), refs[8])
    pipe.run_frames(3, cameras=cams[4:7])
    assert np.array_equal(frame_of(pipe), refs[6])
    pipe.run_frames(2, cameras=cams[1:3])
    assert np.array_equal(frame_of(pipe), refs[2])


@pytest.mark.parametrize("pairing", [1, 2])
def test_static_camera_renders_every_frame(scene, pipe, pairing):
    """No cameras given: all four frames of a group are rendered with the current shader data."""
    r, cams, refs = scene
    pipe.pairing = pairing
    pipe.frame_group = 4
    r.set_shader_data(*cams[5])
    cnt0 = r.get_option("group_launches")
    pipe.run_frames(8)
    assert np.array_equal(frame_of(pipe), refs[5])
    assert r.get_option("group_launches") - cnt0 == 2


@pytest.mark.parametrize("pairing", [1, 2])
def test_switching_frame_group_between_runs(scene, pipe, pairing):
    """2 -> 4 -> 2 with frames queued and not waited for: the switch waits for the pending frames."""
    r, cams, refs = scene
    pipe.pairing = pairing
    pipe.frame_group = 2
    pipe.run_frames(5, cameras=cams[:5])
    pipe.frame_group = 4
    g0, p0 = launches(r)
    pipe.run_frames(6, cameras=cams[:6])
    assert launches(r) == (g0 + 1, p0 + 3)   # one group (two pairs of frames) and a pair
    pipe.frame_group = 2
    pipe.run_frames(4, cameras=cams[3:7])
    assert launches(r) == (g0 + 1, p0 + 5)
    assert np.array_equal(frame_of(pipe), refs[6])
    pipe.frame_group = 4
    pipe.run_frames(4, cameras=cams[:4])
    assert np.array_equal(frame_of(pipe), refs[3])


@pytest.mark.parametrize("pairing", [1, 2])
def test_sampled_groups(scene, pipe, pairing):
    r, cams, refs = scene
    pipe.pairing = pairing
    pipe.frame_group = 4
    ms = pipe.run_frames(9, cameras=cams[:9], sample_every=1)
    assert np.isfinite(ms) and ms > 0.0
    busy, span = pipe.sampled_busy()
    assert 0.0 < busy <= span + 1e-6
    assert np.array_equal(frame_of(pipe), refs[8])


def test_frame_group_range():
    """frame_group is 2 or 4: anything else is VR_ERR_INVALID and leaves the option as it was."""
    from volumetricrenderer_amd._lib import VRError
    with vr.Renderer(0) as r:
        for good in (2, 4, 2, 4):
            r.set_option("frame_group", good)
            assert r.get_option("frame_group") == good
            for bad in (0, 1, 3, 5, 8, -1):
                with pytest.raises(VRError) as e:
                    r.set_option("frame_group", bad)
                assert e.value.status == 1, bad   # VR_ERR_INVALID
                assert r.get_option("frame_group") == good, bad
        # the counters are read-only
        for name in ("group_launches", "pair_launches"):
            with pytest.raises(VRError):
                r.set_option(name, 0)


def test_four_frames_per_launch_is_the_default():
    with vr.Renderer(0) as r:
        assert r.get_option("frame_group") == 4 and r.get_option("frame_pairing") == 2


def test_pairing_off_ignores_frame_group(scene, pipe):
    r, cams, refs = scene
    pipe.pairing = 0
    pipe.frame_group = 4
    g0, p0 = launches(r)
    pipe.run_frames(5, cameras=cams[:5])
    assert np.array_equal(frame_of(pipe), refs[4])
    assert launches(r) == (g0, p0)


H5 = 76   # five 16-row bands: rank 0 of two serpentine renderers holds bands 0, 3 and 4


@pytest.fixture(scope="module")
def tall(scene):
    """(cameras, plain renders of them) for the W x H5 frame of the solo rehearsals, made once."""
    r = scene[0]
    cams = [vr.reference_shader_data(W / H5, 1.6 * i, 15.0) for i in range(3)]
    refs = []
    for c in cams:
        r.set_shader_data(*c)
        refs.append(r.render(W, H5, FMT).cpu().numpy())
    return cams, refs


def own_rows(pl, height, band_rows=16):
    """The frame rows of the pipeline's own band set (vr.h vr_target.band_flip), in the set's order."""
    nb = (height + band_rows - 1) // band_rows
    bands = [b for k in range(nb + 1) for b in [pl.band_first + k * pl.band_stride + (pl.band_flip if k % 2 else 0)]
             if b < nb]
    return [y for b in bands for y in range(b * band_rows, min(height, (b + 1) * band_rows))]


@pytest.mark.parametrize("pairing", [1, 2])
@pytest.mark.parametrize("n", [2, 3])
def test_solo_rank0_pairs_in_place_and_assembles(scene, tall, pairing, n):
    """Rank 0 of two, rehearsed alone: its frames go two at a time into its own rows of the frame
    buffers (in place), each followed by an assembly, an odd last frame alone.  Its band set of the
    last frame equals the same rows of a plain render of that frame's camera."""
    r = scene[0]
    cams, refs = tall
    pl = RcclBandPipeline(r, W, H5, FMT, band_rows=16, world=2, rank=0, loopback=True, solo=True, render_streams=2)
    try:
        pl.pairing = pairing
        assert (pl.band_stride, pl.band_first, pl.band_flip) == (2, 0, 1) and not pl.compositor
        rows = own_rows(pl, H5)
        assert len(rows) == 16 + 16 + 12   # bands 0, 3 and the partial band 4
        assert pl.my_rows == vr.band_rows_packed(H5, 16, 2, 0, 1)
        pl.run_frames(n, cameras=cams[:n])
        got = frame_of(pl)
        assert got.shape == refs[n - 1].shape
        assert np.array_equal(got[rows], refs[n - 1][rows])
    finally:
        pl.close()


def test_solo_compositor_rank0_carries_the_camera(scene, tall):
    """Rank 0 as a compositor without lead rows renders nothing: its rehearsal only assembles, and
    leaves the context with the last frame's shader data, through no shared launch."""
    r = scene[0]
    cams, refs = tall
    pl = RcclBandPipeline(r, W, H5, FMT, band_rows=16, world=2, rank=0, loopback=True, solo=True, compositor=True,
                          render_streams=2, lead_pct=None)
    try:
        assert pl.compositor and pl.my_rows == 0 and pl.lead_rows == 0
        r.set_shader_data(*cams[0])
        g0, p0 = launches(r)
        pl.run_frames(3, cameras=cams[:3])
        assert launches(r) == (g0, p0)
        got = r.render(W, H5, FMT).cpu().numpy()
        assert np.array_equal(got, refs[2])
    finally:
        pl.close()


def test_loopback_ranks_ignore_frame_group():
    """Two ranks in one process: the multi-rank path keeps one launch per frame whatever the options say."""
    Wl, Hl = 500, 283
    with vr.Renderer(0) as r:
        r.generate_volume(vr.volume_recipe_defaults(size=64))
        r.set_shader_data(*vr.reference_shader_data(Wl / Hl, -30.0, 40.0))
        r.set_march(vr.march_defaults())
        full = r.render(Wl, Hl, FMT).cpu().numpy()
        pl = RcclBandPipeline(r, Wl, Hl, FMT, band_rows=16, world=2, rank=0, loopback=True, render_streams=2)
        try:
            pl.pairing = 1
            pl.frame_group = 4
            g0, p0 = launches(r)
            pl.run_frames(5)
            pl.barrier()
            assert np.array_equal(pl.frame().cpu().numpy(), full)
            assert launches(r) == (g0, p0)
        finally:
            pl.close()
