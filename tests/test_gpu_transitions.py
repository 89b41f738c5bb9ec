"""State transitions on one long-lived context: consecutive renders that
differ in exactly one input.

The parity tests re-install the volume, the shader data and the march
constants before every frame and change many inputs at once.  The library
keeps state between frames -- the procedural cost order and its key, the
deferred-shadow ranges sized from it, the region lists and their key, the
per-stream launch cache, the fBm lattice table, the uniform-channel mask, the
layout plan -- and a cache keyed on an incomplete set of inputs shows only when
two consecutive renders differ in the forgotten field alone (as band_flip was
missing from the sort key).  tests/transitions.py holds the harness: apply()
calls only the setters whose inputs changed, check() compares every byte of a
padded, sentinel-filled buffer with the oracle's whole frame and the step
counter with its start value plus the selected rows' steps.

The bar is the project's: bit-exact for the float and UNORM formats, <= 1 LSB
for sRGB, exact step counts.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
# the parameter lists are built without a GPU too, so that every machine
# collects the same test ids
import transitions as T  # noqa: E402


@pytest.fixture(scope="module")
def h(oracle):
    with vr.Renderer(0) as rr:
        yield T.Harness(rr, oracle)


def need_experiments(r, what):
    """Skip unless the library was built with the measured-slower variants."""
    if r.get_option("experiments") != 1:
        pytest.skip(f"{what}: built only with VR_EXPERIMENTS (make EXPERIMENTS=1)")


def test_apply_calls_only_the_setters_that_changed(h):
    """The point of the harness: unchanged state is not installed again."""
    b = T.BASES["G0"]
    h.apply(b, full=True)
    assert h.calls[:5] == ["set_volume", "set_layout_preference", "set_shader_data", "set_march", "set_procedural"]
    assert len(h.calls) == 5 + len(T.OPTION_DEFAULTS)
    for name, want in [("steps47", ["set_march"]), ("phi+1.6", ["set_shader_data"]), ("wedges3", ["set_option:wedges"]),
                       ("flip2", []), ("pad3", []), ("update_box", ["update_volume"]), ("volB", ["set_volume"]),
                       ("layout15", ["set_layout_preference"])]:
        m = next(m for m in T.grid_mutations(0) if m.name == name)
        h.apply(m(b))
        assert h.calls == want, name
        h.apply(b)
        assert len(h.calls) == len(want), name
    h.apply(T.TO_SHADOW(b))
    assert h.calls == ["set_procedural"]
    h.apply(b)
    # ... and a repeated check() of an unchanged grid scene is the same target on the same stream: once the
    # region lists have settled it is served from the launch cache
    hits = h.r.get_option("launch_cache_hits")
    for _ in range(3):
        h.check()
    assert h.r.get_option("launch_cache_hits") > hits


@pytest.mark.parametrize("base,mutation", T.CASES, ids=T.CASE_IDS)
def test_single_change(h, base, mutation):
    """check(B), check(B), check(B + M), check(B): the second render of B goes
    into the same buffer, refilled, so the launch cache and the reuse paths
    (SORT_REUSE, exact region lists) are taken; the last one proves the way
    back as clean as the way out."""
    b = T.ALL_BASES[base]
    s = mutation(b)
    if T.needs_experiments(s):
        need_experiments(h.r, mutation.name)
    h.apply(b, full=True)
    h.check()
    h.check()
    h.apply(s)
    if mutation.name == "scroll_out":
        assert h.r.kernel_variant == "grid_planar_mirror"
    elif mutation.name == "scroll_in" and b.layout != 1:
        assert "_clamp" in h.r.kernel_variant
    h.check()
    h.apply(b)
    h.check()


@pytest.mark.parametrize("family", sorted(T.WALKS))
def test_random_walk(h, family):
    """A seeded walk of one or two random mutations per step from the current
    scene: orderings the single-change walks do not reach."""
    base, scenes = T.walk(family)
    h.apply(base, full=True)
    h.check()
    for i, s in enumerate(scenes):
        h.apply(s)
        try:
            h.check()
        except AssertionError as e:
            raise AssertionError(f"step {i}: {scenes[i - 1] if i else base} -> {s}: {e}") from e
