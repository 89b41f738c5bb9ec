"""The transform paste -- vr_stamp_affine and vr_clone_affine -- restated in
numpy (include/vr.h), and what the affine tests share.

`spec_affine` follows the header line by line: positions in int64, the outside
test, the clamp, the nearest texel, and the trilinear value as ONE sum over the
eight corners of wx wy wz byte in uint32 (the library factors it; here it is
not).  The inside mask, the weights and the clipped box are paint_spec's, the
three blends clone_spec's; nothing is shared with the library.

The volume is paint_spec.base_volume() (37 x 22 x 45 random bytes) and the
brushes are paint_spec.BRUSHES.  Every 16.16 table of MAPS is written out; a
map is placed by its pivot (the brush centre) and the source position that the
pivot lands on (`src`, in texels: the brush centre again for a clone, the
middle of the stamp for a stamp).
"""
import numpy as np

import clone_spec as cs
import paint_spec as ps

NEAREST, LINEAR = 0, 1
CLAMP, SKIP = 0, 1
FILTERS = [(NEAREST, "nearest"), (LINEAR, "linear")]
ONE = 65536
I3 = ((ONE, 0, 0), (0, ONE, 0), (0, 0, ONE))
STRENGTH = ps.STRENGTH
FULL = cs.FULL

STAMP_EXTENT = (13, 9, 11)   # bx, by, bz of the stamp the stamp tests paste
STAMP_CENTRE = (6, 4, 5)


def _at(src, shift=(0, 0, 0)):
    """The 16.16 origin: the source texel `src` plus a 16.16 shift."""
    return tuple(int(s) * ONE + int(d) for s, d in zip(src, shift))


# name -> f(pivot, src) = (m, pivot, origin): 16.16 tables, written out
MAPS = {
    "identity": lambda c, s: (I3, c, _at(s)),
    "shift_int": lambda c, s: (I3, c, _at(s, (5 * ONE, -3 * ONE, 7 * ONE))),
    "shift_half": lambda c, s: (I3, c, _at(s, (0x8000, 0x4000, 0))),
    "rot90_z": lambda c, s: (((0, -65536, 0), (65536, 0, 0), (0, 0, 65536)), c, _at(s)),
    # the inverse of the rotation by 30 degrees about (1, 1, 2) / sqrt(6), times 65536, rounded
    "rot30_axis": lambda c, s: (((58219, 28218, -10451), (-25292, 58219, 16304), (16304, -10451, 62609)), c, _at(s)),
    "scale2": lambda c, s: (((32768, 0, 0), (0, 32768, 0), (0, 0, 32768)), c, _at(s)),       # the copy twice as large
    "half": lambda c, s: (((131072, 0, 0), (0, 131072, 0), (0, 0, 131072)), c, _at(s)),     # the copy half as large
    "shear": lambda c, s: (((65536, 16384, 0), (0, 65536, -32768), (8192, 0, 65536)), c, _at(s)),
    "flip": lambda c, s: (((-65536, 0, 0), (0, 65536, 0), (0, 0, 65536)), c, _at(s)),
    "collapse": lambda c, s: (((0, 0, 0), (0, 0, 0), (0, 0, 0)), c, _at(s, (0x2000, 0xC000, 0x8000))),
    # 25 texels up z: with `interior` (z 19..27 of 45) the clone reads z = 44 only -- the direct path
    "far": lambda c, s: (I3, c, _at(s, (0, 0, 25 * ONE))),
    # the pivot lands on source x = -0.25: the texels left of the brush centre are outside the source
    "off_source": lambda c, s: (I3, c, (-0x4000,) + _at(s)[1:]),
}
BORDERS = {name: ((CLAMP, SKIP) if name in ("off_source", "shift_int") else (CLAMP,)) for name in MAPS}


def rot30():
    """The rotation whose inverse rot30_axis spells out, for the builder tests."""
    k = np.array([1.0, 1.0, 2.0]) / np.sqrt(6.0)
    t = np.radians(30.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def stamp_bytes(extent=STAMP_EXTENT, seed=131):
    bx, by, bz = extent
    return np.random.default_rng(seed).integers(0, 256, size=(bz, by, bx, 4), dtype=np.uint8)


def positions(table, shape):
    """P_x, P_y, P_z (int64, shaped (nz, ny, nx)) of every destination texel of a (nz, ny, nx) volume."""
    m, pivot, origin = table
    nz, ny, nx = shape
    t = [np.arange(n, dtype=np.int64) - np.int64(p) for n, p in zip((nx, ny, nz), pivot)]
    tx, ty, tz = t[0][None, None, :], t[1][None, :, None], t[2][:, None, None]
    return [np.int64(origin[a]) + np.int64(m[a][0]) * tx + np.int64(m[a][1]) * ty + np.int64(m[a][2]) * tz for a in range(3)]


def sample(src, table, filt, shape):
    """(v, outside): the value v[z, y, x, c] (int64) of every destination texel of a (nz, ny, nx) volume, read from
    `src` (bz, by, bx, 4) at the CLAMPED position, and which texels are outside the source."""
    n = src.shape[2::-1]   # n_x, n_y, n_z
    P = positions(table, shape)
    outside = np.zeros(shape, bool)
    for a in range(3):
        last = np.int64(n[a] - 1) << np.int64(16)
        outside |= (P[a] < 0) | (P[a] > last)
        P[a] = np.clip(P[a], 0, last)
    i = [p >> np.int64(16) for p in P]
    if filt == NEAREST:
        s = [ia + ((p & np.int64(0xFFFF)) >= 0x8000) for ia, p in zip(i, P)]
        assert all((sa <= na - 1).all() for sa, na in zip(s, n))
        return src[s[2], s[1], s[0], :].astype(np.int64), outside
    f = [((p >> np.int64(8)) & np.int64(255)).astype(np.uint32) for p in P]
    j = [np.minimum(ia + 1, na - 1) for ia, na in zip(i, n)]
    acc = np.zeros(shape + (4,), np.uint32)
    total = np.zeros(shape, np.uint32)
    for corner in range(8):
        idx, w = [], np.ones(shape, np.uint32)
        for a in range(3):
            second = corner >> a & 1
            idx.append(j[a] if second else i[a])
            w = w * (f[a] if second else np.uint32(256) - f[a])
        total += w
        acc += w[..., None] * src[idx[2], idx[1], idx[0], :].astype(np.uint32)
    assert (total == 1 << 24).all()
    return ((acc + np.uint32(1 << 23)) >> np.uint32(24)).astype(np.int64), outside


def spec_affine(vol, src, table, filt, border, centre, radius, op, falloff, strength=STRENGTH, sampled=None):
    """The pasted copy of `vol` (nz, ny, nx, 4); `src` is the stamp, or None for the volume itself as it was.
    `sampled` = sample(...) of the same source, map and filter, when the caller has it already."""
    source = vol if src is None else src
    v, outside = sampled if sampled is not None else sample(source, table, filt, vol.shape[:3])
    inside, w = ps.spec_weights(vol.shape[:3], centre, radius, falloff)
    touched = inside & ~outside if border == SKIP else inside
    out = vol.copy()
    for c in range(4):
        if strength[c] == 0:
            continue
        old = vol[..., c].astype(np.int64)
        out[..., c] = np.where(touched, cs.blend(op, old, v[..., c], w * strength[c]), old).astype(np.uint8)
    return out


def spec_direct(table, filt, centre, radius, dims=(ps.NX, ps.NY, ps.NZ)):
    """The path rule of vr_clone_affine, restated: True for the direct path."""
    m, pivot, origin = table
    box = ps.spec_box(centre, radius, dims)
    assert box is not None
    o, e = box
    for a in range(3):
        P = []
        for k in range(8):
            t = [o[b] + (e[b] - 1 if k >> b & 1 else 0) for b in range(3)]
            P.append(origin[a] + sum(m[a][b] * (t[b] - pivot[b]) for b in range(3)))   # Python ints: exact
        lo, hi = min(P), max(P)
        r0, r1 = (lo >> 16, (hi >> 16) + 1) if filt == LINEAR else ((lo + 0x8000) >> 16, (hi + 0x8000) >> 16)
        r0, r1 = (min(max(r, 0), dims[a] - 1) for r in (r0, r1))
        if r1 < o[a] or r0 > o[a] + e[a] - 1:
            return True
    return False


def reads_a_written_texel(table, filt, border, centre, radius, dims=(ps.NX, ps.NY, ps.NZ)):
    """Brute force: does a texel the clone writes (inside the ellipsoid and processed) get read by one of them?"""
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    P = positions(table, shape)
    outside = np.zeros(shape, bool)
    for a in range(3):
        last = np.int64(dims[a] - 1) << np.int64(16)
        outside |= (P[a] < 0) | (P[a] > last)
        P[a] = np.clip(P[a], 0, last)
    inside, _ = ps.spec_weights(shape, centre, radius, 0)
    written = inside & ~outside if border == SKIP else inside
    i = [p >> np.int64(16) for p in P]
    if filt == NEAREST:
        taps = [[ia + ((p & np.int64(0xFFFF)) >= 0x8000) for ia, p in zip(i, P)]]
    else:
        j = [np.minimum(ia + 1, na - 1) for ia, na in zip(i, dims)]
        taps = [[(j[a] if k >> a & 1 else i[a]) for a in range(3)] for k in range(8)]
    read = np.zeros(shape, bool)
    for sx, sy, sz in taps:
        read[sz[written], sy[written], sx[written]] = True
    return bool((read & written).any())
