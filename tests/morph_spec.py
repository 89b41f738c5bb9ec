"""The erode / dilate brush of vr_morph restated in numpy (include/vr.h;
DESIGN.md sec. 5.2.9), and what the morph tests share.

`spec_morph` pads the volume by the half width with `np.pad(mode="edge")` --
clamp-to-edge -- and takes the extremum over the (2h + 1)^3 cube with
`np.minimum.reduce` / `np.maximum.reduce` over shifted views, one axis after
the other, all from the bytes before the call (Jacobi).  The inside mask and
the weights are paint_spec's; nothing is shared with the library.

The input is NOT paint_spec.base_volume(): on uniformly random bytes a 7^3
minimum is 0 almost everywhere and a wrong window passes.  `morph_volume` is a
ramp with a little noise on it, bytes 0..254, on which the half widths, an
in-place sweep and (for erode) a zero padding all give other bytes.
"""
import numpy as np

import paint_spec as ps

ERODE, DILATE = 0, 1
OPS = [(ERODE, "erode"), (DILATE, "dilate")]
HALF_WIDTHS = (1, 2, 3)
STRENGTH = ps.STRENGTH   # (255, 128, 1, 0): a full, a partial and a faint channel, and one left alone
FULL = (255, 255, 255, 255)


def morph_volume():
    """37 x 22 x 45: ((3x + 2y + 4z + 40c) % 224) + (base_volume() >> 3)."""
    z, y, x, c = np.meshgrid(np.arange(ps.NZ), np.arange(ps.NY), np.arange(ps.NX), np.arange(4), indexing="ij")
    return (((3 * x + 2 * y + 4 * z + 40 * c) % 224) + (ps.base_volume() >> 3)).astype(np.uint8)


def cube_extrema(channel, h, op, pad_mode="edge"):
    """The minimum (ERODE) / maximum (DILATE) over the (2h + 1)^3 cube of every texel of `channel` (nz, ny, nx)."""
    reduce = np.maximum.reduce if op == DILATE else np.minimum.reduce
    s = np.pad(channel.astype(np.int64), h, mode=pad_mode)
    for axis in range(3):
        n = s.shape[axis] - 2 * h
        s = reduce([np.take(s, np.arange(k, k + n), axis=axis) for k in range(2 * h + 1)])
    return s


def spec_morph(vol, centre, radius, op, h, falloff, strength=STRENGTH):
    """The eroded / dilated copy of `vol` (nz, ny, nx, 4)."""
    inside, w = ps.spec_weights(vol.shape[:3], centre, radius, falloff)
    out = vol.copy()
    for c in range(4):
        if strength[c] == 0:
            continue
        old = vol[..., c].astype(np.int64)
        m = cube_extrema(vol[..., c], h, op)
        a = w * strength[c]
        new = (old * (65280 - a) + m * a + 32640) // 65280
        out[..., c] = np.where(inside, new, old).astype(np.uint8)
    return out


def clamped_axes(shape, centre, radius, h):
    """Per inside texel, on how many axes its cube leaves the volume (0..3); -1 outside the brush."""
    inside, _ = ps.spec_weights(shape, centre, radius, 0)
    nz, ny, nx = shape
    idx = [np.arange(n) for n in (nx, ny, nz)]
    cl = [(i < h) | (i > n - 1 - h) for i, n in zip(idx, (nx, ny, nz))]
    count = cl[0][None, None, :].astype(int) + cl[1][None, :, None] + cl[2][:, None, None]
    return np.where(inside, count, -1)


def gauss_seidel_morph(vol, op, h):
    """What an IN-PLACE sweep (z, y, x ascending) of a hard, full-strength, whole-volume morph leaves: each
    extremum sees the bytes the sweep has already written.  Not the specification -- what a wrong implementation
    gives."""
    out = vol.copy()
    nz, ny, nx, _ = out.shape
    off = np.arange(-h, h + 1)
    pick = np.max if op == DILATE else np.min
    for z in range(nz):
        zs = np.clip(z + off, 0, nz - 1)
        for y in range(ny):
            ys = np.clip(y + off, 0, ny - 1)
            for x in range(nx):
                xs = np.clip(x + off, 0, nx - 1)
                out[z, y, x] = pick(out[np.ix_(zs, ys, xs)].reshape(-1, 4), axis=0)
    return out
