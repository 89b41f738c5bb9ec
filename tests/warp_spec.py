"""The liquify brush -- vr_warp -- restated in numpy (include/vr.h; DESIGN.md
sec. 5.2.15), and what the warp tests share.

`spec_warp` follows the header line by line: the affine position A and the
texel's own position I in int64, D = A - I, P = I + ((w * D) >> 8) with numpy's
arithmetic shift (floor), then the outside test, the clamp, the nearest texel
and the trilinear value as ONE sum over the eight corners in uint32, and the
SET blend with a = 256 * strength.  The inside mask, the weights and the
clipped box are paint_spec's, the blend clone_spec's, the affine positions
affine_spec's; nothing is shared with the library.

The volume is paint_spec.base_volume(), the brushes paint_spec.BRUSHES and the
maps affine_spec.MAPS placed with pivot = src = the brush centre, plus a push
by a fraction of a texel, a twirl and a pinch, whose 16.16 tables are written
out.  `tile_footprint` restates which source texels each 8 x 8 x 8 tile of the
clipped box reads -- what decides the device path of a tile.
"""
import numpy as np

import affine_spec as af
import clone_spec as cs
import paint_spec as ps

NEAREST, LINEAR, CLAMP, SKIP = af.NEAREST, af.LINEAR, af.CLAMP, af.SKIP
FILTERS = af.FILTERS
BORDERS = [(CLAMP, "clamp"), (SKIP, "skip")]
ONE = af.ONE
STRENGTH = af.STRENGTH   # (255, 128, 1, 0): the mixed strengths of the affine tests
FULL = af.FULL
MAX_DISP16 = 32768 << 16   # VR_WARP_MAX_DISP << 16
TILE = 8
BUDGET = 4096              # texels of a tile's footprint that go through LDS


def _minus(origin, d):
    return tuple(int(o) - int(v) for o, v in zip(origin, d))


MAPS = dict(af.MAPS)
MAPS.update({
    # the content moves by (+1.5, -0.5, +0.25) texels
    "push_frac": lambda c, s: (af.I3, c, _minus(af._at(s), (0x18000, -0x8000, 0x4000))),
    # the inverse of the rotation by 20 degrees about z, times 65536, rounded: cos 20 = 0.93969262, sin 20 = 0.34202014
    "twirl20": lambda c, s: (((61584, 22415, 0), (-22415, 61584, 0), (0, 0, 65536)), c, af._at(s)),
    # the content shrinks to 0.8 of its size: the inverse is 1.25
    "pinch": lambda c, s: (((81920, 0, 0), (0, 81920, 0), (0, 0, 81920)), c, af._at(s)),
    # the content shrinks to a quarter: a full tile reads 29 texels per axis, far over the LDS budget
    "quarter": lambda c, s: (((262144, 0, 0), (0, 262144, 0), (0, 0, 262144)), c, af._at(s)),
})

# With the hard `whole` brush (w = 256, P = A) about its centre (18, 11, 22): twice the texel offset plus half a texel.
# The tile x 16..23, y 8..15, z 16..23 reads 16 texels per axis -- exactly BUDGET -- and no tile reads more.
BUDGET_EXACT = (((131072, 0, 0), (0, 131072, 0), (0, 0, 131072)), (18, 11, 22), af._at((18, 11, 22), (0x8000, 0x8000, 0x8000)))
# the same with y scaled by 2.15: that tile reads y 5..21, one row of texels more: 16 x 17 x 16 = BUDGET + 256
BUDGET_OVER = (((131072, 0, 0), (0, 140902, 0), (0, 0, 131072)), (18, 11, 22), af._at((18, 11, 22), (0x8000, 0x8000, 0x8000)))


def placed(mname, centre):
    return MAPS[mname](centre, centre)


def positions(table, shape, w):
    """P_x, P_y, P_z (int64, shaped (nz, ny, nx)) of every texel of a (nz, ny, nx) volume under the weights w."""
    nz, ny, nx = shape
    A = af.positions(table, shape)
    t = [np.arange(n, dtype=np.int64) for n in (nx, ny, nz)]
    I = [t[0][None, None, :] << np.int64(16), t[1][None, :, None] << np.int64(16), t[2][:, None, None] << np.int64(16)]
    w = w.astype(np.int64)
    return [I[a] + ((w * (A[a] - I[a])) >> np.int64(8)) for a in range(3)]


def clamped(P, dims):
    """(clamped positions, outside mask) on a volume of dims = (nx, ny, nz)."""
    outside = np.zeros(P[0].shape, bool)
    out = []
    for a in range(3):
        last = np.int64(dims[a] - 1) << np.int64(16)
        outside |= (P[a] < 0) | (P[a] > last)
        out.append(np.clip(P[a], 0, last))
    return out, outside


def texels(P, filt, dims):
    """Per axis (first, last, f): the texels a clamped position reads and, LINEAR, the weight of the second."""
    r = []
    for a in range(3):
        i = P[a] >> np.int64(16)
        if filt == NEAREST:
            s = i + ((P[a] & np.int64(0xFFFF)) >= 0x8000)
            r.append((s, s, None))
        else:
            f = (P[a] >> np.int64(8)) & np.int64(255)
            j = np.where((f == 0) | (i + 1 > dims[a] - 1), i, i + 1)   # a second texel of weight 0 is the first again
            r.append((i, j, f.astype(np.uint32)))
    return r


def sample_at(src, P, filt):
    """The value v[z, y, x, c] (int64) read from `src` (nz, ny, nx, 4) at the clamped positions P."""
    dims = src.shape[2::-1]
    tx = texels(P, filt, dims)
    if filt == NEAREST:
        return src[tx[2][0], tx[1][0], tx[0][0], :].astype(np.int64)
    shape = P[0].shape
    acc = np.zeros(shape + (4,), np.uint32)
    total = np.zeros(shape, np.uint32)
    for corner in range(8):
        idx, w = [], np.ones(shape, np.uint32)
        for a in range(3):
            second = corner >> a & 1
            idx.append(tx[a][1] if second else tx[a][0])
            w = w * (tx[a][2] if second else np.uint32(256) - tx[a][2])
        total += w
        acc += w[..., None] * src[idx[2], idx[1], idx[0], :].astype(np.uint32)
    assert (total == 1 << 24).all()
    return ((acc + np.uint32(1 << 23)) >> np.uint32(24)).astype(np.int64)


def spec_warp(vol, table, filt, border, centre, radius, falloff, strength=STRENGTH):
    """The warped copy of `vol` (nz, ny, nx, 4): every value is read from `vol`, never from the copy."""
    shape = vol.shape[:3]
    dims = shape[::-1]
    inside, w = ps.spec_weights(shape, centre, radius, falloff)
    P, outside = clamped(positions(table, shape, w), dims)
    v = sample_at(vol, P, filt)
    touched = inside & ~outside if border == SKIP else inside
    out = vol.copy()
    for c in range(4):
        if strength[c] == 0:
            continue
        old = vol[..., c].astype(np.int64)
        out[..., c] = np.where(touched, cs.blend(ps.SET, old, v[..., c], np.int64(256 * strength[c])), old).astype(np.uint8)
    return out


def spec_reach(table, centre, radius):
    """max |D_a| per axis over the 8 corners of the unclipped box, in Python ints (exact)."""
    m, pivot, origin = table
    r = [0, 0, 0]
    for k in range(8):
        t = [centre[b] + (radius[b] if k >> b & 1 else -radius[b]) for b in range(3)]
        for a in range(3):
            A = origin[a] + sum(m[a][b] * (t[b] - pivot[b]) for b in range(3))
            r[a] = max(r[a], abs(A - t[a] * 65536))
    return tuple(r)


def tile_footprint(table, filt, centre, radius, falloff, dims=(ps.NX, ps.NY, ps.NZ), border=CLAMP):
    """Per 8 x 8 x 8 tile of the clipped box, x fastest: (ex, ey, ez), the extent of the box of source texels its
    touched texels read (both texels of a LINEAR position, the nearest of a NEAREST one), or None for a tile without
    a touched texel.  An empty list when the brush misses the volume."""
    box = ps.spec_box(centre, radius, dims)
    if box is None:
        return []
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    inside, w = ps.spec_weights(shape, centre, radius, falloff)
    P, outside = clamped(positions(table, shape, w), dims)
    touched = inside & ~outside if border == SKIP else inside
    tx = texels(P, filt, dims)
    (ox, oy, oz), (bx, by, bz) = box
    out = []
    for z0 in range(oz, oz + bz, TILE):
        for y0 in range(oy, oy + by, TILE):
            for x0 in range(ox, ox + bx, TILE):
                sl = (slice(z0, min(z0 + TILE, oz + bz)), slice(y0, min(y0 + TILE, oy + by)), slice(x0, min(x0 + TILE, ox + bx)))
                m = touched[sl]
                if not m.any():
                    out.append(None)
                    continue
                out.append(tuple(int(np.broadcast_to(tx[a][1], shape)[sl][m].max() - np.broadcast_to(tx[a][0], shape)[sl][m].min()) + 1
                                 for a in range(3)))
    return out


def volumes(fp):
    """The texel counts of the tiles that read anything."""
    return [e[0] * e[1] * e[2] for e in fp if e is not None]
