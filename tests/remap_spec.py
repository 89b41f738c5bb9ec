"""The lookup-table brush -- vr_remap -- and its four table builders restated in
numpy (include/vr.h), and what the remap tests share.

Everything is int64.  The inside mask, the weights and the clipped box are
paint_spec's (`spec_weights`, `spec_box`); the three blends are restated in
`blend`; nothing is shared with the library.

The base volume is paint_spec.base_volume() (37 x 22 x 45 random bytes: every
byte value occurs about 475 times per channel, so a table entry that is wrong
for one byte value shows).  The SKEWED volume is that volume with each channel
squared, divided by 255 (dark bytes become common, bright ones rare, so
equalising differs from stretching) and confined to a sub-range (so stretching
differs from the identity); its G is constant (the single-bin rule).
"""
import numpy as np

import paint_spec as ps

FULL = (255, 255, 255, 255)
ZERO_CHANNEL = (255, 0, 128, 255)      # a strength vector with a zero channel: G is neither read nor written
EQUALIZE, STRETCH = 0, 1
SKEW_G = 77
# channel -> (lowest byte, span) of the skewed volume: byte = lowest + (b * b // 255) * span // 255
SKEW_RANGE = {0: (20, 180), 2: (40, 100), 3: (5, 200)}
STATS_BRUSH = ("whole", 1)             # the brush (name, falloff) whose stats of the skewed volume give `eq` and `stretch`


def blend(op, old, v, a):
    """include/vr.h: the new byte of a channel, a = w * strength (int64 arrays)."""
    d = (v * a + 32640) // 65280
    if op == ps.SET:
        return (old * (65280 - a) + v * a + 32640) // 65280
    if op == ps.ADD:
        return np.minimum(255, old + d)
    return np.maximum(0, old - d)


def spec_remap(vol, lut, centre, radius, op, falloff, strength=ps.STRENGTH):
    """The remapped copy of `vol` (nz, ny, nx, 4): the value of a texel's channel c is lut[c][its old byte]."""
    inside, w = ps.spec_weights(vol.shape[:3], centre, radius, falloff)
    lut = np.asarray(lut).astype(np.int64)
    out = vol.copy()
    for c in range(4):
        if strength[c] == 0:
            continue
        old = vol[..., c].astype(np.int64)
        out[..., c] = np.where(inside, blend(op, old, lut[c][old], w * strength[c]), old).astype(np.uint8)
    return out


def spec_identity():
    return np.tile(np.arange(256, dtype=np.int64), (4, 1)).astype(np.uint8)


def spec_levels(lut, mask, in_lo, in_hi, out_lo, out_hi):
    """vr_lut_levels on a copy of `lut`: python's // floors, also for a negative numerator."""
    out = np.asarray(lut).copy()
    v = np.arange(256, dtype=np.int64)
    den = in_hi - in_lo
    mid = out_lo + (2 * (v - in_lo) * (out_hi - out_lo) + den) // (2 * den)
    row = np.where(v <= in_lo, out_lo, np.where(v >= in_hi, out_hi, mid))
    assert row.min() >= 0 and row.max() <= 255
    for c in range(4):
        if mask >> c & 1:
            out[c] = row.astype(np.uint8)
    return out


def spec_compose(first, then):
    first, then = np.asarray(first), np.asarray(then)
    return np.stack([then[c][first[c].astype(np.int64)] for c in range(4)]).astype(np.uint8)


def spec_stats_lut(hist, kind, mask):
    """vr_stats_lut from the (4, 256) histograms (python ints: nothing can overflow)."""
    out = spec_identity()
    for c in range(4):
        h = [int(x) for x in hist[c]]
        nonzero = [v for v in range(256) if h[v]]
        if not (mask >> c & 1) or len(nonzero) < 2:
            continue
        lo, hi, n, cmin = nonzero[0], nonzero[-1], sum(h), h[nonzero[0]]
        cum = 0
        for v in range(256):
            cum += h[v]
            if kind == STRETCH:
                e = 0 if v <= lo else 255 if v >= hi else ((v - lo) * 255 + (hi - lo) // 2) // (hi - lo)
            else:
                e = 0 if v < lo else ((cum - cmin) * 255 + (n - cmin) // 2) // (n - cmin)
            assert 0 <= e <= 255
            out[c][v] = e
    return out


def skewed_volume():
    b = ps.base_volume().astype(np.int64)
    sq = b * b // 255
    out = np.empty_like(b)
    for c, (lowest, span) in SKEW_RANGE.items():
        out[..., c] = lowest + sq[..., c] * span // 255
    out[..., 1] = SKEW_G
    return out.astype(np.uint8)


def spec_hist(vol, centre, radius, strength=FULL):
    """The (4, 256) histograms of vr_brush_stats: the inside texels of each channel with a non-zero strength."""
    inside, _ = ps.spec_weights(vol.shape[:3], centre, radius, 0)
    hist = np.zeros((4, 256), np.int64)
    for c in range(4):
        if strength[c]:
            hist[c] = np.bincount(vol[..., c][inside], minlength=256)
    return hist


def _perm():
    """A fixed-seed permutation per channel, the four different, none with a fixed point anywhere (so not at the
    volume's most common bytes either): a derangement, drawn again until it is one."""
    rng = np.random.default_rng(20241020)
    rows = []
    while len(rows) < 4:
        p = rng.permutation(256)
        if (p != np.arange(256)).all():
            rows.append(p)
    return np.stack(rows).astype(np.uint8)


def tables():
    """name -> (4, 256) uint8 table"""
    ident = spec_identity()
    hist = spec_hist(skewed_volume(), *ps.BRUSHES[STATS_BRUSH[0]])
    posterise = np.tile(np.arange(256, dtype=np.int64) & 0xC0, (4, 1)).astype(np.uint8)
    return {
        "perm": _perm(),
        "invert": spec_levels(ident, 15, 0, 255, 255, 0),
        "thresh128": spec_levels(ident, 15, 127, 128, 0, 255),
        "levels_narrow": spec_levels(ident, 15, 40, 90, 10, 240),
        "posterise": posterise,
        "identity": ident,
        "eq": spec_stats_lut(hist, EQUALIZE, 15),
        "stretch": spec_stats_lut(hist, STRETCH, 15),
    }


TABLES = tables()
