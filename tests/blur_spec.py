"""The smoothing brush of vr_blur restated in numpy (include/vr.h; DESIGN.md
sec. 5.2.7), and what the blur tests share.

`spec_blur` pads the volume by the half width with `np.pad(mode="edge")` --
clamp-to-edge -- and forms the (2h + 1)^3 sums as shifted sums in int64, one
axis after the other, all from the bytes before the call (Jacobi).  The inside
mask and the weights are paint_spec's; nothing is shared with the library.
"""
import numpy as np

import paint_spec as ps

HALF_WIDTHS = (1, 2, 3)
STRENGTH = ps.STRENGTH   # (255, 128, 1, 0): a full, a partial and a faint channel, and one left alone


def box_sums(channel, h):
    """int64 sums over the (2h + 1)^3 neighbourhood of every texel of `channel` (nz, ny, nx), clamp-to-edge."""
    s = np.pad(channel.astype(np.int64), h, mode="edge")
    for axis in range(3):
        n = s.shape[axis] - 2 * h
        s = sum(np.take(s, np.arange(k, k + n), axis=axis) for k in range(2 * h + 1))
    return s


def box_means(channel, h):
    n = (2 * h + 1) ** 3
    return (box_sums(channel, h) + n // 2) // n


def spec_blur(vol, centre, radius, h, falloff, strength=STRENGTH):
    """The blurred copy of `vol` (nz, ny, nx, 4)."""
    inside, w = ps.spec_weights(vol.shape[:3], centre, radius, falloff)
    out = vol.copy()
    for c in range(4):
        if strength[c] == 0:
            continue
        old = vol[..., c].astype(np.int64)
        m = box_means(vol[..., c], h)
        a = w * strength[c]
        new = (old * (65280 - a) + m * a + 32640) // 65280
        out[..., c] = np.where(inside, new, old).astype(np.uint8)
    return out


def clamped_axes(shape, centre, radius, h):
    """Per inside texel, on how many axes its neighbourhood leaves the volume (0..3); -1 outside the brush."""
    inside, _ = ps.spec_weights(shape, centre, radius, 0)
    nz, ny, nx = shape
    idx = [np.arange(n) for n in (nx, ny, nz)]
    cl = [(i < h) | (i > n - 1 - h) for i, n in zip(idx, (nx, ny, nz))]
    count = cl[0][None, None, :].astype(int) + cl[1][None, :, None] + cl[2][:, None, None]
    return np.where(inside, count, -1)


def gauss_seidel_blur(vol, h):
    """What an IN-PLACE sweep (z, y, x ascending) of a hard, full-strength, whole-volume blur leaves: each mean
    sees the bytes the sweep has already written.  Not the specification -- what a wrong implementation gives."""
    out = vol.copy()
    nz, ny, nx, _ = out.shape
    n = (2 * h + 1) ** 3
    off = np.arange(-h, h + 1)
    for z in range(nz):
        zs = np.clip(z + off, 0, nz - 1)
        for y in range(ny):
            ys = np.clip(y + off, 0, ny - 1)
            for x in range(nx):
                xs = np.clip(x + off, 0, nx - 1)
                s = out[np.ix_(zs, ys, xs)].reshape(-1, 4).sum(axis=0, dtype=np.int64)
                out[z, y, x] = (s + n // 2) // n
    return out
