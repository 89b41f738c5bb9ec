"""The conditions of the edit chain (tests/edit_chain.py, test_gpu_edit_chain.py), checked with the
oracle and numpy alone so that they hold before any kernel runs: every edit changes the expected
volume and the oracle's frame, the fill's region is neither empty nor everything, the uniform mask
goes through kept, kept after the same-value write, and lost, the order is the one the module states,
the early-out ends rays at each of the four positions of a step round, and some ray has more than 8
steps."""
import numpy as np
import pytest

import edit_chain as ec
import fill_spec as fs

VARIANTS = pytest.mark.parametrize("variant", ec.VARIANTS, ids=ec.VARIANT_IDS)
FAMILY = {"update_volume", "paint", "paint_stroke", "blur", "morph", "rank", "clone", "stamp", "remap", "stamp_affine",
          "clone_affine", "fill"}


@VARIANTS
def test_one_edit_per_family_member_in_the_stated_order(variant):
    edits, vols = ec.expected(variant)
    assert len(edits) == 12 and {e.name for e in edits} == FAMILY
    assert len(vols) == 13 and all(v.shape == (ec.DIMS[2], ec.DIMS[1], ec.DIMS[0], 4) and v.dtype == np.uint8 for v in vols)
    assert ec.truly_uniform(vols[0]) == (0 if variant is None else 1 << variant)
    # (a) the staged brushes alternate between the large and the small box, and the large one is the larger
    staged = [e for e in edits if e.name in ec.STAGED]
    sizes = [ec.STAGED[e.name] for e in staged]
    assert sizes == ["large", "small"] * 3
    texels = [int(np.prod(e.boxes[0][1])) for e in staged]
    assert min(t for t, s in zip(texels, sizes) if s == "large") > max(t for t, s in zip(texels, sizes) if s == "small")
    # every edit's boxes meet the boxes of the edit before it
    for a, b in zip(edits, edits[1:]):
        assert any(ec.boxes_meet(x, y) for x in a.boxes for y in b.boxes), (a.name, b.name)
    assert [e.phase for e in edits] == ec.PHASES
    assert [e.name for e in edits if e.phase in "cde" and e.phase] == ["paint", "stamp", "update_volume"]


@VARIANTS
def test_every_edit_changes_the_volume(variant):
    edits, vols = ec.expected(variant)
    for i, e in enumerate(edits):
        changed = (vols[i] != vols[i + 1]).any(axis=3)
        assert changed.any(), f"step {i + 1} {e.name}: the expected volume is unchanged"
        # ... and only inside its boxes
        inside = np.zeros(changed.shape, bool)
        for (x, y, z), (bx, by, bz) in e.boxes:
            inside[z:z + bz, y:y + by, x:x + bx] = True
        assert not (changed & ~inside).any(), f"step {i + 1} {e.name}: texels outside {e.boxes} changed"


@VARIANTS
def test_every_edit_changes_the_oracles_frame(oracle, variant):
    edits, vols = ec.expected(variant)
    counts = []
    for i, e in enumerate(edits):
        n = [int((ec.oracle_frame(oracle, vols[i], 0, early) != ec.oracle_frame(oracle, vols[i + 1], 0, early)).any(axis=2).sum())
             for early in (0.0, ec.EARLY)]
        counts.append((i + 1, e.name, n))
    print("changed pixels per edit (early-out 0, early-out on):", counts)
    for step, name, n in counts:
        assert n[0] > 0, f"step {step} {name}: changed pixels of camera 0 (early-out 0, on) {n}; all edits {counts}"
    assert sum(n[1] > 0 for _, _, n in counts) >= 8, f"with the early-out on too few edits show: {counts}"


@VARIANTS
def test_the_fills_region(variant):
    edits, vols = ec.expected(variant)
    i = [e.name for e in edits].index("fill")
    c, r = ec.BRUSHES["wide"]
    passable, region, report = fs.spec_region(vols[i], c, r, ec.fill_rule(c))
    inside = int(ec.ps.spec_weights(vols[i].shape[:3], c, r, 0)[0].sum())
    assert 1 < report[0] == int(region.sum()) and report[1] == int(passable.sum()) < inside, (report, inside)


@VARIANTS
def test_mask_trajectory(variant):
    """Kept through (b), kept after (c) wrote the uniform byte itself, lost at (d), and still lost after (e) made
    the channel constant again (it is then truly uniform, which the library does not look for)."""
    edits, vols = ec.expected(variant)
    want = 0 if variant is None else 1 << variant
    masks = [ec.expected_mask(variant, k) for k in range(13)]
    assert all(a & b == b for a, b in zip(masks, masks[1:]))       # monotone
    for k, e in enumerate(edits, 1):
        assert masks[k] == (want if e.phase in ("b", "c") else 0), (k, e.name, masks)
        assert masks[k] & ~ec.truly_uniform(vols[k]) == 0
    q = ec.quiet(variant)
    c5 = [e.phase for e in edits].index("c")
    # (c) really writes channel q: its strength there is full and the value is the uniform byte
    painted = ec.ps.spec_apply(vols[c5], *ec.BRUSHES["wide"], ec.ps.SET, 1, (1, 2, 3, 4), ec.FULL)
    assert (painted[..., q] != vols[c5][..., q]).any()
    if variant is not None:
        assert (vols[c5 + 1][..., q] == ec.UVAL).all()
        assert ec.truly_uniform(vols[c5 + 2]) == 0                                   # (d)
    assert ec.truly_uniform(vols[12]) == 1 << q and (vols[12][..., q] == ec.UVAL_AGAIN).all()   # (e)
    assert masks[12] == 0


@VARIANTS
def test_early_out_lands_on_every_step_of_a_round(oracle, variant):
    """At every step of the chain ec.EARLY ends rays after 4k + 1, 4k + 2, 4k + 3 and 4k + 4 steps, short of their
    own end (each lane's position in a round of the QUAD kernels' step rounds): the condition of
    test_gpu_quad_pairs.py's test of the same name, from the oracle's step totals (ec.early_out_cuts; the counts
    are lower bounds)."""
    edits, vols = ec.expected(variant)
    for k, vol in enumerate(vols):
        cuts, full = ec.early_out_cuts(oracle, vol, 0, ec.EARLY)
        residues = [sum(cuts[j] for j in range(1, ec.STEPS + 1) if j % 4 == m) for m in (1, 2, 3, 0)]
        assert all(n > 0 for n in residues), f"after {k} edits: rays ended by steps % 4 = 1, 2, 3, 0: {residues}; by step {cuts}"
    # and early-out 0.05, were it used, would end none: the bound is not trivially positive
    assert sum(ec.early_out_cuts(oracle, vols[0], 0, 0.05)[0]) == 0


def test_some_ray_has_more_than_eight_steps(oracle):
    """At step_scale 1: the step rounds' second refill runs (two rounds and more)."""
    for cam in range(len(ec.CAMERAS)):
        obj, glob = ec.shader_arrays(cam)
        n = oracle.step_counts(obj, glob, oracle.from_params(ec.march_params()), ec.W, ec.H)
        assert n.max() == ec.STEPS > 8 and (n > 8).sum() > 100
        assert len({int(v) % 4 for v in n[n > 0]}) == 4     # every tail length of a round
        assert n.shape == (ec.H, ec.W) and ec.W % 2 == 0 and ec.W % 8 and ec.H % 2   # quads fall off both edges


def test_the_cameras_differ(oracle):
    vol = ec.expected(None)[1][0]
    frames = [ec.oracle_frame(oracle, vol, cam) for cam in range(4)]
    assert all((frames[0] != f).any() for f in frames[1:])
    assert (frames[0][..., 0] > 0).sum() > 300
