"""The brushes whose value is a texel -- vr_clone and vr_stamp -- restated in
numpy (include/vr.h), and what the clone tests share.

`spec_clone` and `spec_stamp` follow the header line by line.  The inside mask,
the weights and the clipped box are paint_spec's (`spec_weights`, `spec_box`);
the three blends are restated in `blend`; nothing is shared with the library.
Source coordinates are int64, so any int32 offset is exact before the clamp.

The volume is paint_spec.base_volume() (37 x 22 x 45 random bytes: a texel and
its neighbour differ almost surely, so a source off by one texel, an in-place
sweep and a missing clamp all give other bytes) and the brushes are
paint_spec.BRUSHES.
"""
import numpy as np

import paint_spec as ps

STRENGTH = ps.STRENGTH   # (255, 128, 1, 0): a full, a partial and a faint channel, and one left alone
FULL = (255, 255, 255, 255)
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31

# name -> f(centre) = (offset, mirror).  Stated for the brush `interior` (centre (17, 11, 23), radius (3, 2, 4):
# box x 14..20); only mirror_xyz follows the centre of the brush in use.
MAPS = {
    "far": lambda c: ((12, 0, 0), (0, 0, 0)),         # source x 26..32: the direct path
    "touch": lambda c: ((7, 0, 0), (0, 0, 0)),        # source x 21..27, adjacent to the box: still direct
    "overlap1": lambda c: ((6, 0, 0), (0, 0, 0)),     # source x 20..26, one shared column: staged
    "push+x": lambda c: ((1, 0, 0), (0, 0, 0)),       # an in-place sweep in any order gets one of each pair wrong
    "push-x": lambda c: ((-1, 0, 0), (0, 0, 0)),
    "push+y": lambda c: ((0, 1, 0), (0, 0, 0)),
    "push-y": lambda c: ((0, -1, 0), (0, 0, 0)),
    "push+z": lambda c: ((0, 0, 1), (0, 0, 0)),
    "push-z": lambda c: ((0, 0, -1), (0, 0, 0)),
    "mirror_x": lambda c: ((34, 0, 0), (1, 0, 0)),    # about the plane x = 17
    "mirror_xyz": lambda c: (tuple(2 * v for v in c), (1, 1, 1)),   # about the brush centre
    "edge": lambda c: ((-30, 40, -60), (0, 0, 0)),    # the source clamps to the corner (0, ny - 1, 0)
    "huge": lambda c: ((INT32_MAX, INT32_MIN, 0), (0, 0, 0)),   # the clamp is taken in 64 bits
    "identity": lambda c: ((0, 0, 0), (0, 0, 0)),     # SET leaves every byte as it was
}
DIRECT_MAPS = ("far", "touch", "edge", "huge")        # with `interior`: the source range misses the box on an axis
PUSHES = ("push+x", "push-x", "push+y", "push-y", "push+z", "push-z")


def blend(op, old, v, a):
    """include/vr.h: the new byte of a channel, a = w * strength (int64 arrays)."""
    d = (v * a + 32640) // 65280
    if op == ps.SET:
        return (old * (65280 - a) + v * a + 32640) // 65280
    if op == ps.ADD:
        return np.minimum(255, old + d)
    return np.maximum(0, old - d)


def source_index(n, offset, mirror):
    """s_a for t_a = 0..n-1: mirror ? offset - t : t + offset, clamped to [0, n - 1]."""
    t = np.arange(n, dtype=np.int64)
    s = (np.int64(offset) - t) if mirror else (t + np.int64(offset))
    return np.clip(s, 0, n - 1)


def spec_clone(vol, centre, radius, offset, mirror, op, falloff, strength=STRENGTH):
    """The cloned copy of `vol` (nz, ny, nx, 4): every value is read from `vol`, never from the copy."""
    nz, ny, nx = vol.shape[:3]
    inside, w = ps.spec_weights(vol.shape[:3], centre, radius, falloff)
    sx, sy, sz = (source_index(n, o, m) for n, o, m in zip((nx, ny, nz), offset, mirror))
    out = vol.copy()
    for c in range(4):
        if strength[c] == 0:
            continue
        old = vol[..., c].astype(np.int64)
        v = vol[sz[:, None, None], sy[None, :, None], sx[None, None, :], c].astype(np.int64)
        out[..., c] = np.where(inside, blend(op, old, v, w * strength[c]), old).astype(np.uint8)
    return out


def spec_direct(centre, radius, offset, mirror, dims=(ps.NX, ps.NY, ps.NZ)):
    """True when the clamped source range of the clipped box misses the box on at least one axis."""
    box = ps.spec_box(centre, radius, dims)
    assert box is not None
    for a in range(3):
        s = source_index(dims[a], offset[a], mirror[a])[box[0][a]:box[0][a] + box[1][a]]
        if s.max() < box[0][a] or s.min() > box[0][a] + box[1][a] - 1:
            return True
    return False


def spec_stamp_box(centre, radius, origin, extent, dims=(ps.NX, ps.NY, ps.NZ)):
    """(origin, extent) of the clipped brush box intersected with the placement, or None."""
    box = ps.spec_box(centre, radius, dims)
    if box is None:
        return None
    lo = [max(b, p) for b, p in zip(box[0], origin)]
    hi = [min(b + e, p + q) for b, e, p, q in zip(box[0], box[1], origin, extent)]   # one past the end
    if any(a >= b for a, b in zip(lo, hi)):
        return None
    return tuple(lo), tuple(b - a for a, b in zip(lo, hi))


def spec_stamp(vol, stamp, origin, centre, radius, op, falloff, strength=STRENGTH):
    """The stamped copy of `vol`: `stamp` (bz, by, bx, 4) lies with its first texel on volume texel `origin`;
    a texel is touched iff it is inside the ellipsoid, the volume and the placement."""
    nz, ny, nx = vol.shape[:3]
    bz, by, bx = stamp.shape[:3]
    inside, w = ps.spec_weights(vol.shape[:3], centre, radius, falloff)
    idx = [np.arange(n, dtype=np.int64) - np.int64(o) for n, o in zip((nx, ny, nz), origin)]   # stamp coordinates
    cov = [(i >= 0) & (i < b) for i, b in zip(idx, (bx, by, bz))]
    covered = cov[0][None, None, :] & cov[1][None, :, None] & cov[2][:, None, None]
    ix, iy, iz = (np.clip(i, 0, b - 1) for i, b in zip(idx, (bx, by, bz)))
    touched = inside & covered
    out = vol.copy()
    for c in range(4):
        if strength[c] == 0:
            continue
        old = vol[..., c].astype(np.int64)
        v = stamp[iz[:, None, None], iy[None, :, None], ix[None, None, :], c].astype(np.int64)
        out[..., c] = np.where(touched, blend(op, old, v, w * strength[c]), old).astype(np.uint8)
    return out


def sweep_clone(vol, centre, radius, offset, ascending=True):
    """What an IN-PLACE sweep (z, y, x ascending or descending) of a hard, full-strength SET clone leaves: a value
    may be a byte the sweep has already written.  Not the specification -- what a wrong implementation gives."""
    nz, ny, nx = vol.shape[:3]
    inside, _ = ps.spec_weights(vol.shape[:3], centre, radius, 0)
    out = vol.copy()
    order = np.argwhere(inside)
    for z, y, x in (order if ascending else order[::-1]):
        s = [int(np.clip(t + o, 0, n - 1)) for t, o, n in zip((x, y, z), offset, (nx, ny, nz))]
        out[z, y, x] = out[s[2], s[1], s[0]]
    return out


# stamp cases on the base volume: name -> (brush name, stamp extent (bx, by, bz), placement origin (x, y, z))
STAMPS = {
    "covers": ("interior", (9, 7, 11), (13, 8, 18)),          # the placement holds the whole brush box
    "two_faces": ("corner", (8, 9, 6), (-3, -4, 1)),           # hangs over the faces x = 0 and y = 0
    "far_faces": ("far_corner", (7, 5, 9), (33, 19, 40)),      # hangs over the far faces
    "smaller": ("straddle", (5, 3, 2), (18, 9, 30)),           # a placement smaller than the brush
    "miss": ("interior", (3, 3, 3), (25, 11, 23)),             # in the volume, beside the brush box: nothing edited
    "outside": ("whole", (4, 4, 4), (INT32_MAX - 3, INT32_MIN, 40)),   # x + bx is formed in 64 bits
    "one": ("interior", (1, 1, 1), (17, 11, 23)),              # a 1 x 1 x 1 stamp on the centre
    "max": ("max", (37, 22, 45), (0, 0, 0)),                   # the whole volume through the largest brush
}


def stamp_bytes(extent, seed=77):
    bx, by, bz = extent
    return np.random.default_rng(seed).integers(0, 256, size=(bz, by, bx, 4), dtype=np.uint8)
