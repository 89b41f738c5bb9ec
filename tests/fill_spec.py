"""The flood-fill brush of vr_fill restated in numpy (include/vr.h; DESIGN.md
sec. 5.2.14), and what the fill tests share.  Nothing is shared with the
library: there is no queue and no union-find here.

`spec_fill` takes paint_spec's inside mask and weights, the passable mask from
the rule (the seed's bytes, the per-channel ranges), and finds the region by
repeated 6-neighbour dilation of the seed mask ANDed with `passable` until it
stops growing; the blend is paint_spec's on the region only.  A rule is a
`Rule(seed, lo, hi, select, relative)`; a report is `(filled, passable, min,
max)` with the empty one `(0, 0, (nx, ny, nz), (-1, -1, -1))`.

The volumes, 37 x 22 x 45 like paint_spec's (4*8+5, 2*8+6, 5*8+5: every axis
cuts the labelling's 8-tiles); the field a rule tests is in R, and A holds 255
- R so that a rule on A tests the lower bound where one on R tests the upper;
G and B are paint_spec's random bytes.
  * blobs: R = 128 + 42 (sin 0.45 x' + sin 0.6 y' + sin 0.35 z') rounded,
    passable where R >= 175: the sum must pass 1.12, which no two sines reach
    while the third is at its lowest, so the maxima are separate blobs.  Seeds
    hold >= 230.  Under `whole` the region of the seed nearest the centre holds
    more than 5 % and less than 60 % of the passable texels (494 of 7674).
  * snakes: two interleaved one-texel corridors, a two-lane road that runs in
    serpentines through every even z plane and steps to the next plane at its
    end.  Corridor bytes run through 100..140 (both ends occur), every other
    texel -- the walls -- holds exactly 141 = hi + 1 (A: 114 = lo - 1).  Each
    corridor holds more than 40 % of the passable texels under `whole`, the two
    are disjoint, and `snakes()` returns their texel lists in path order.
  * detour: two passable parts inside the `interior` brush, joined only by a
    path that leaves the ellipsoid; only the seed's part fills.
  * edges: R = (9 x + 5 y + 3 z) mod 256, relative distances 10 / 10 around
    seeds that hold 0, 3 and 252, so the range clamps at 0 and at 255.
One larger volume, 70 x 33 x 41 = 94 710 texels, holds the snakes again: a
label of 16 bits or a row index that overflows cannot pass it.
"""
from typing import NamedTuple

import numpy as np

import paint_spec as ps

NX, NY, NZ = ps.NX, ps.NY, ps.NZ
LARGE = (70, 33, 41)
STRENGTH = ps.STRENGTH   # (255, 128, 1, 0): A is never painted
FULL = (255, 255, 255, 255)
VALUE = ps.VALUE
SNAKE_LO, SNAKE_HI, SNAKE_WALL = 100, 140, 141
BLOB_LEVEL, BLOB_SEED_LEVEL = 175, 230


class Rule(NamedTuple):
    seed: tuple
    lo: tuple
    hi: tuple
    select: tuple = (1, 0, 0, 0)
    relative: int = 1


def empty_report(dims):
    return 0, 0, tuple(dims), (-1, -1, -1)


# ---- the specification ------------------------------------------------------------------------
def passable_mask(vol, centre, radius, rule):
    """(nz, ny, nx) bool: inside the brush and, per selected channel, inside the rule's range."""
    inside, _ = ps.spec_weights(vol.shape[:3], centre, radius, 0)
    sx, sy, sz = rule.seed
    ok = inside.copy()
    for c in range(4):
        if not rule.select[c]:
            continue
        b = vol[..., c].astype(np.int64)
        if rule.relative:
            s = int(vol[sz, sy, sx, c])
            lo, hi = max(0, s - rule.lo[c]), min(255, s + rule.hi[c])
        else:
            lo, hi = rule.lo[c], rule.hi[c]
        ok &= (b >= lo) & (b <= hi)
    return ok


def grow(passable, seed):
    """The region: the seed mask dilated along the six axis directions, ANDed with `passable`, to its fixed point."""
    region = np.zeros(passable.shape, bool)
    sx, sy, sz = seed
    region[sz, sy, sx] = passable[sz, sy, sx]
    count = int(region.sum())
    while count:
        d = region.copy()
        d[1:] |= region[:-1]; d[:-1] |= region[1:]
        d[:, 1:] |= region[:, :-1]; d[:, :-1] |= region[:, 1:]
        d[:, :, 1:] |= region[:, :, :-1]; d[:, :, :-1] |= region[:, :, 1:]
        d &= passable
        n = int(d.sum())
        if n == count:
            break
        region, count = d, n
    return region


_regions = {}


def spec_region(vol, centre, radius, rule):
    """(passable, region, report), computed once per (volume, brush, rule); callers leave them unchanged.  A brush
    that misses the volume and a seed outside the clipped box give no passable texel and the empty report."""
    key = (vol.shape, hash(vol.tobytes()), tuple(centre), tuple(radius), rule)
    if key not in _regions:
        nz, ny, nx = vol.shape[:3]
        box = ps.spec_box(centre, radius, (nx, ny, nz))
        if box is None or any(not o <= s < o + e for s, o, e in zip(rule.seed, *box)):
            none = np.zeros(vol.shape[:3], bool)
            _regions[key] = (none, none, empty_report((nx, ny, nz)))
        else:
            passable = passable_mask(vol, centre, radius, rule)
            region = grow(passable, rule.seed)
            report = empty_report((nx, ny, nz))
            if region.any():
                z, y, x = np.nonzero(region)
                report = (int(region.sum()), 0, (int(x.min()), int(y.min()), int(z.min())), (int(x.max()), int(y.max()), int(z.max())))
            _regions[key] = (passable, region, (report[0], int(passable.sum())) + report[2:])
        for a in _regions[key][:2]:
            a.setflags(write=False)
    return _regions[key]


def spec_fill(vol, centre, radius, op, falloff, rule, value=VALUE, strength=STRENGTH):
    """(the filled copy of `vol` (nz, ny, nx, 4), the report)."""
    _, region, report = spec_region(vol, centre, radius, rule)
    painted = ps.spec_apply(vol, centre, radius, op, falloff, value, strength)
    return np.where(region[..., None], painted, vol), report


# ---- the volumes ------------------------------------------------------------------------------
def _with_field(field, dims=(NX, NY, NZ)):
    nx, ny, nz = dims
    vol = np.random.default_rng(ps.SEED).integers(0, 256, size=(nz, ny, nx, 4), dtype=np.uint8)
    vol[..., 0] = field
    vol[..., 3] = 255 - field.astype(np.int64)
    return vol


def blobs():
    z, y, x = np.meshgrid(np.arange(NZ), np.arange(NY), np.arange(NX), indexing="ij")
    f = np.sin(0.45 * x + 0.3) + np.sin(0.6 * y + 1.1) + np.sin(0.35 * z + 2.0)
    return _with_field(np.clip(np.rint(128 + 42 * f), 0, 255).astype(np.uint8))


def snake_paths(dims=(NX, NY, NZ)):
    """The texel lists [(x, y, z), ...] of the two corridors, in path order.  In an even z plane pass j of the road
    holds the rows y = 4 j and y = 4 j + 2; at a turn the outer lane runs on to the last column and round to the far
    row of the next pass, the inner lane turns two columns earlier into the near one.  Every plane holds the same
    road, walked forwards in planes 0, 4, ... and backwards in planes 2, 6, ...; the two lanes step through the odd
    plane between at the road's end (or start)."""
    nx, ny, nz = dims
    passes = (ny - 3) // 4 + 1
    lanes = ([], [])   # the road of one plane: the lane that starts on row 0, the lane that starts on row 2
    for lane in (0, 1):
        row, x = 2 * lane, 0
        for j in range(passes):
            right, last = j % 2 == 0, j == passes - 1
            near = row == 4 * j                    # on the row nearer the previous pass: the outer lane of the turn ahead
            end = nx - 1 if right else 0
            if not (last or near):
                end += -2 if right else 2
            step = 1 if right else -1
            lanes[lane].extend((xx, row) for xx in range(x, end + step, step))
            x = end
            if last:
                break
            nxt = 4 * (j + 1) + (2 if near else 0)
            lanes[lane].extend((x, y) for y in range(row + 1, nxt))
            row = nxt
    paths = ([], [])
    for k, z in enumerate(range(0, nz, 2)):
        for lane in (0, 1):
            road = lanes[lane] if k % 2 == 0 else lanes[lane][::-1]
            paths[lane].extend((x, y, z) for x, y in road)
            if z + 2 < nz:
                paths[lane].append((road[-1][0], road[-1][1], z + 1))
    return paths


def snakes(dims=(NX, NY, NZ)):
    """(volume, corridor A's texels, corridor B's texels)."""
    nx, ny, nz = dims
    field = np.full((nz, ny, nx), SNAKE_WALL, np.uint8)
    a, b = snake_paths(dims)
    for path, phase in ((a, 0), (b, 17)):
        for i, (x, y, z) in enumerate(path):
            field[z, y, x] = SNAKE_LO + (7 * i + phase) % (SNAKE_HI - SNAKE_LO + 1)
    return _with_field(field, dims), a, b


DETOUR_PARTS = ([(x, y, z) for x in (15, 16) for y in (10, 11, 12) for z in (22, 23, 24)],
                [(x, y, z) for x in (18, 19) for y in (10, 11, 12) for z in (22, 23, 24)])


def detour():
    """Two blocks either side of the wall x = 17 inside `interior` ((17, 11, 23), (3, 2, 4)), joined by a path over
    y = 15, outside the brush's box (|dy| <= 2)."""
    field = np.zeros((NZ, NY, NX), np.uint8)
    for x, y, z in DETOUR_PARTS[0] + DETOUR_PARTS[1]:
        field[z, y, x] = 200
    for x in (15, 19):
        field[23, 12:16, x] = 200
    field[23, 15, 15:20] = 200
    return _with_field(field)


def edges():
    z, y, x = np.meshgrid(np.arange(NZ), np.arange(NY), np.arange(NX), indexing="ij")
    return _with_field(((9 * x + 5 * y + 3 * z) % 256).astype(np.uint8))


EDGE_SEED_BYTES = (0, 3, 252)


def nearest(candidates, centre, dims=(NX, NY, NZ)):
    """The texel of `candidates` ((n, 3) x, y, z) nearest to `centre` clamped to the volume (ties: the first)."""
    c = np.array([min(max(v, 0), n - 1) for v, n in zip(centre, dims)])
    cand = np.asarray(candidates)
    return tuple(int(v) for v in cand[np.argmin(((cand - c) ** 2).sum(axis=1))])


def texels_where(mask):
    z, y, x = np.nonzero(mask)
    return np.stack([x, y, z], axis=1)


def relative_rule(vol, seed, lo_abs, hi_abs, channel=0):
    """The relative rule on `channel` that allows exactly lo_abs..hi_abs around the seed's byte (which lies inside)."""
    s = int(vol[seed[2], seed[1], seed[0], channel])
    lo, hi, sel = [0] * 4, [0] * 4, [0] * 4
    lo[channel], hi[channel], sel[channel] = s - lo_abs, hi_abs - s, 1
    return Rule(tuple(seed), tuple(lo), tuple(hi), tuple(sel), 1)


def absolute_rule(seed, lo_abs, hi_abs, channel=0):
    lo, hi, sel = [0] * 4, [0] * 4, [0] * 4
    lo[channel], hi[channel], sel[channel] = lo_abs, hi_abs, 1
    return Rule(tuple(seed), tuple(lo), tuple(hi), tuple(sel), 0)


class Case(NamedTuple):
    """A volume with, per brush, the seed to use and the rule in both forms."""
    vol: np.ndarray
    candidates: np.ndarray    # (n, 3) texels a seed is taken from: the nearest to the brush's centre
    lo_abs: int
    hi_abs: int
    channel: int = 0

    def seed(self, centre):
        return nearest(self.candidates, centre, self.vol.shape[2::-1])

    def rule(self, centre, relative, channel=None):
        """The rule around the seed for the brush at `centre`; on channel A the range is the mirrored one."""
        ch = self.channel if channel is None else channel
        lo, hi = (self.lo_abs, self.hi_abs) if ch == 0 else (255 - self.hi_abs, 255 - self.lo_abs)
        s = self.seed(centre)
        return relative_rule(self.vol, s, lo, hi, ch) if relative else absolute_rule(s, lo, hi, ch)


def cases():
    """name -> Case.  A relative rule allows the same bytes as the absolute one, stated around the seed's byte."""
    bl = blobs()
    sn, a, b = snakes()
    dt = detour()
    ed = edges()
    return {
        "blobs": Case(bl, texels_where(bl[..., 0] >= BLOB_SEED_LEVEL), BLOB_LEVEL, 255),
        "snakes": Case(sn, np.array(a + b), SNAKE_LO, SNAKE_HI),
        "detour": Case(dt, np.array(DETOUR_PARTS[0]), 200, 200),
        "edges": Case(ed, texels_where(np.isin(ed[..., 0], EDGE_SEED_BYTES)), 0, 0),
    }


def edge_rule(vol, seed):
    """edges: distances 10 below and 10 above the seed's byte, whatever it is -- the range clamps at 0 and 255."""
    return Rule(tuple(seed), (10, 0, 0, 0), (10, 0, 0, 0), (1, 0, 0, 0), 1)
