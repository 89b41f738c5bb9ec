"""The median / rank-filter brush of vr_rank restated in numpy (include/vr.h;
DESIGN.md sec. 5.2.12), and what the rank tests share.

`cube_sorted` pads a channel by the half width with `np.pad(mode="edge")` --
clamp-to-edge, so a clamped texel counts once for every offset that lands on
it -- stacks the (2h + 1)^3 shifted views and sorts along the last axis;
`spec_rank` takes index `rank` of it and blends with paint_spec's inside mask
and weights, all from the bytes before the call (Jacobi).  Nothing is shared
with the library: there is no bisection here.

Two inputs, both 37 x 22 x 45:
  * morph_spec.morph_volume(), a ramp with noise, on which neighbouring ranks,
    the half widths, a zero-padded halo and a separable median of medians all
    give other bytes (test_rank_cpu.py asserts the fractions);
  * tie_volume(): four distinct bytes, 0, 1, 128 and 255, so nearly every
    window is full of ties, the bisection meets the candidate 1 and the result
    255, and a `<=`-for-`<` count shows.
"""
import numpy as np

import morph_spec as ms
import paint_spec as ps

MEDIAN = -1
HALF_WIDTHS = (1, 2, 3)
STRENGTH = ps.STRENGTH   # (255, 128, 1, 0): a full, a partial and a faint channel, and one left alone
FULL = (255, 255, 255, 255)


def window(h):
    return (2 * h + 1) ** 3


def resolve(rank, h):
    return (window(h) - 1) // 2 if rank == MEDIAN else rank


def tie_volume():
    return np.array([0, 1, 128, 255], np.uint8)[ps.base_volume() >> 6]


INPUTS = [("ramp", ms.morph_volume), ("ties", tie_volume)]

_sorted = {}


def cube_sorted(channel, h, pad_mode="edge"):
    """(nz, ny, nx, N) uint8: every texel's (2h + 1)^3 clamped neighbours of `channel` (nz, ny, nx), ascending.
    Computed once per (bytes, h, padding) and shared; callers must leave it unchanged."""
    key = (channel.shape, channel.tobytes(), h, pad_mode)
    if key not in _sorted:
        s = np.pad(channel, h, mode=pad_mode)
        nz, ny, nx = channel.shape
        views = [s[dz:dz + nz, dy:dy + ny, dx:dx + nx]
                 for dz in range(2 * h + 1) for dy in range(2 * h + 1) for dx in range(2 * h + 1)]
        out = np.sort(np.stack(views, axis=-1), axis=-1)
        out.setflags(write=False)
        _sorted[key] = out
    return _sorted[key]


def cube_rank(channel, h, rank, pad_mode="edge"):
    """The rank-th smallest (0-based; MEDIAN: the middle) of every texel's cube, (nz, ny, nx) int64."""
    return cube_sorted(channel, h, pad_mode)[..., resolve(rank, h)].astype(np.int64)


def spec_rank(vol, centre, radius, rank, h, falloff, strength=STRENGTH):
    """The rank-filtered copy of `vol` (nz, ny, nx, 4)."""
    inside, w = ps.spec_weights(vol.shape[:3], centre, radius, falloff)
    out = vol.copy()
    for c in range(4):
        if strength[c] == 0:
            continue
        old = vol[..., c].astype(np.int64)
        m = cube_rank(np.ascontiguousarray(vol[..., c]), h, rank)
        a = w * strength[c]
        new = (old * (65280 - a) + m * a + 32640) // 65280
        out[..., c] = np.where(inside, new, old).astype(np.uint8)
    return out


def separable_median(channel, h):
    """The median over x of the median over y... in the order x, y, z: NOT the specification -- what a kernel
    gives that treats the rank as the blur and the morph treat their windows."""
    s = channel
    for axis in (2, 1, 0):
        pad = [(0, 0)] * 3
        pad[axis] = (h, h)
        p = np.pad(s, pad, mode="edge")
        n = s.shape[axis]
        s = np.sort(np.stack([np.take(p, np.arange(k, k + n), axis=axis) for k in range(2 * h + 1)], axis=-1), axis=-1)[..., h]
    return s.astype(np.int64)


def wrong_rule_rank(channel, h, rank):
    """A bisection that counts neighbours `<= cand` where the rule counts `< cand`: NOT the specification."""
    srt = cube_sorted(channel, h)
    k = resolve(rank, h)
    lo = np.zeros(channel.shape, np.int64)
    for bit in (128, 64, 32, 16, 8, 4, 2, 1):
        cand = lo | bit
        below = (srt <= cand[..., None].astype(np.uint8)).sum(axis=-1)
        lo = np.where(below <= k, cand, lo)
    return lo
