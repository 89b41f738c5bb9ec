"""The brush of vr_paint restated in numpy, and the inputs the paint tests share.

`spec_apply` follows include/vr.h line by line, with
uint64 for Q and S; it shares no code with the library.  The volume is the
37 x 22 x 45 one of test_gpu_update.py (no axis a multiple of a brick edge).
"""
import numpy as np

NX, NY, NZ = 37, 22, 45
SEED = 20240607
VALUE = (200, 60, 255, 10)
STRENGTH = (255, 128, 1, 0)
SET, ADD, SUB = 0, 1, 2
OPS = [(SET, "set"), (ADD, "add"), (SUB, "sub")]
FALLOFFS = [(0, "hard"), (1, "smooth")]

# name -> (centre (x, y, z), radius (rx, ry, rz))
BRUSHES = {
    "interior": ((17, 11, 23), (3, 2, 4)),
    "texel": ((17, 11, 23), (0, 0, 0)),
    "corner": ((0, 0, 0), (5, 5, 5)),
    "far_corner": ((36, 21, 44), (5, 3, 6)),
    "outside_centre": ((-2, 10, 47), (4, 4, 4)),
    # crosses a brick boundary of every layout on every axis: x 3..35, y 6..14 (7 | 8), z 29..33 (30 | 31, 31 | 32)
    "straddle": ((19, 10, 31), (16, 4, 2)),
    "whole": ((18, 11, 22), (40, 40, 40)),
    "max": ((18, 11, 22), (255, 255, 255)),
    "miss": ((-10, -10, -10), (4, 4, 4)),
}


def base_volume():
    return np.random.default_rng(SEED).integers(0, 256, size=(NZ, NY, NX, 4), dtype=np.uint8)


def spec_box(centre, radius, dims=(NX, NY, NZ)):
    """(origin, extent) of [centre - radius, centre + radius] clipped to the volume, or None."""
    lo = [max(0, c - r) for c, r in zip(centre, radius)]
    hi = [min(n - 1, c + r) for c, r, n in zip(centre, radius, dims)]
    if any(a > b for a, b in zip(lo, hi)):
        return None
    return tuple(lo), tuple(b - a + 1 for a, b in zip(lo, hi))


def spec_weights(shape, centre, radius, falloff):
    """(inside mask, weights) over a (nz, ny, nx) volume; weights are 0 outside."""
    nz, ny, nx = shape
    d = [np.arange(n, dtype=np.int64) - c for n, c in zip((nx, ny, nz), centre)]
    dx, dy, dz = d[0][None, None, :], d[1][None, :, None], d[2][:, None, None]
    box = (np.abs(dx) <= radius[0]) & (np.abs(dy) <= radius[1]) & (np.abs(dz) <= radius[2])
    # outside the bounding box the products could pass 2^64: clamp the offsets there (those texels are masked anyway)
    cl = [(np.uint64(2) * np.minimum(np.abs(v), r).astype(np.uint64)) ** 2 for v, r in zip((dx, dy, dz), radius)]
    D2 = [np.uint64((2 * r + 1) ** 2) for r in radius]
    S = D2[0] * D2[1] * D2[2]
    Q = cl[0] * (D2[1] * D2[2]) + cl[1] * (D2[0] * D2[2]) + cl[2] * (D2[0] * D2[1])
    inside = box & (Q <= S)
    if falloff:
        w = np.uint64(256) - (np.uint64(256) * np.where(inside, Q, np.uint64(0))) // (S + np.uint64(1))
    else:
        w = np.full(Q.shape, 256, np.uint64)
    return inside, np.where(inside, w, np.uint64(0)).astype(np.int64)


def spec_apply(vol, centre, radius, op, falloff, value=VALUE, strength=STRENGTH):
    """The painted copy of `vol` (nz, ny, nx, 4)."""
    inside, w = spec_weights(vol.shape[:3], centre, radius, falloff)
    out = vol.copy()
    for c in range(4):
        if strength[c] == 0:
            continue
        old = vol[..., c].astype(np.int64)
        a = w * strength[c]
        d = (value[c] * a + 32640) // 65280
        if op == SET:
            new = (old * (65280 - a) + value[c] * a + 32640) // 65280
        elif op == ADD:
            new = np.minimum(255, old + d)
        else:
            new = np.maximum(0, old - d)
        out[..., c] = np.where(inside, new, old).astype(np.uint8)
    return out
