"""The statistics of vr_brush_stats / vr_box_stats restated in numpy (include/vr.h;
DESIGN.md sec. 5.2.8), and what the stats tests share.

The inside mask and the weights are paint_spec.spec_weights'; the sums are
`np.bincount` over the bytes the mask selects.  Nothing is shared with the
library.  A result is a dict: count, weight (python ints), wsum (4,) and hist
(4, 256) as int64 arrays.
"""
import numpy as np

import paint_spec as ps

STRENGTHS = [(255, 128, 1, 0), (0, 0, 0, 255)]
FULL = (255, 255, 255, 255)


def _sums(vol, inside, w, selected):
    out = dict(count=int(inside.sum()), weight=int(w[inside].sum()), wsum=np.zeros(4, np.int64),
               hist=np.zeros((4, 256), np.int64))
    for c in range(4):
        if not selected[c]:
            continue
        b = vol[..., c][inside].astype(np.int64)
        out["hist"][c] = np.bincount(b, minlength=256)
        out["wsum"][c] = int((b * w[inside]).sum())
    return out


def spec_brush_stats(vol, centre, radius, falloff, strength):
    inside, w = ps.spec_weights(vol.shape[:3], centre, radius, falloff)
    return _sums(vol, inside, w, [s != 0 for s in strength])


def spec_box_stats(vol, origin, extent, mask):
    inside = np.zeros(vol.shape[:3], bool)
    (x0, y0, z0), (bx, by, bz) = origin, extent
    inside[z0:z0 + bz, y0:y0 + by, x0:x0 + bx] = True
    return _sums(vol, inside, np.where(inside, 256, 0).astype(np.int64), [(mask >> c) & 1 for c in range(4)])


def spec_summary(st):
    """n, min, max, mean, wmean, median per channel from the byte lists the histogram stands for."""
    out = {k: np.zeros(4, np.int64) for k in ("n", "min", "max", "mean", "wmean", "median")}
    for c in range(4):
        b = np.repeat(np.arange(256), np.asarray(st["hist"][c], np.int64))   # ascending
        n = len(b)
        out["n"][c] = n
        if n == 0:
            continue
        out["min"][c], out["max"][c] = b.min(), b.max()
        out["mean"][c] = (int(b.sum()) + n // 2) // n
        out["wmean"][c] = (int(st["wsum"][c]) + int(st["weight"]) // 2) // int(st["weight"])
        out["median"][c] = b[(n + 1) // 2 - 1]   # the smallest v with 2 cum(v) >= n: the ceil(n / 2)-th byte
    return out


def assert_stats(got, want, what=""):
    """`got` is the library's Stats (count, weight, wsum, hist), `want` a dict of this module."""
    assert int(got.count) == want["count"], (what, "count", int(got.count), want["count"])
    assert int(got.weight) == want["weight"], (what, "weight", int(got.weight), want["weight"])
    assert got.wsum.shape == (4,) and got.hist.shape == (4, 256)
    assert np.array_equal(got.wsum.astype(np.int64), want["wsum"]), (what, "wsum", got.wsum, want["wsum"])
    bad = np.argwhere(got.hist.astype(np.int64) != want["hist"])
    assert bad.size == 0, (what, f"{len(bad)} bins differ, first {bad[:5].tolist()}")
