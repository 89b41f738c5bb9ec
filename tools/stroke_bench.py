#!/usr/bin/env python3
"""Cost of a brush stroke in one launch (vr_paint_stroke) against the same dabs as K vr_paint
calls, the path before it.

A 512^3 recipe volume on the auto layout; a smooth ADD brush; strokes of 16 and 64 dabs along
the volume's diagonal at radius 8, spacing 4 and at radius 32, spacing 8 (vr_brush_line).  Per
stroke:

  stroke   one vr_paint_stroke: 1 paint launch, at most 8 layout rebuilds;
  paints   K vr_paint calls on the same stream: K paint launches, K layout rebuilds.

Each is timed with device events on one otherwise idle stream after warm-up calls of the same
shape; the table gives the median, the minimum and the maximum, the median on the host clock
beside them, and the ratio of the medians.  The uniform channel of the recipe is broken by one
texel first, so every timed call is the steady state: launches only.  Before every call the
stroke's bounding box is restored from device memory (vr_update_volume_device, outside the
events), so every call paints the same bytes.  After the timings each path is run once more from
those bytes: both must leave identical bytes, and the bytes of the CPU loop of vr_brush_apply.
Nothing is gated: the numbers are a record.

    python tools/stroke_bench.py [--size 512] [--reps 25] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import volumetricrenderer_amd as vr  # noqa: E402
from volumetricrenderer_amd import _lib  # noqa: E402

VALUE, STRENGTH = (40, 25, 60, 10), (255, 128, 64, 255)
STROKES = [(8, 4, 16), (8, 4, 64), (32, 8, 16), (32, 8, 64)]   # radius, spacing, dabs


def timed(fn, before, stream, warmup, reps):
    """Milliseconds of each of `reps` calls of fn() on `stream`: (device events, host clock
    from before the call until its end event has completed).  before() is queued on the stream
    ahead of every call, outside the events."""
    for _ in range(warmup):
        before()
        fn()
    stream.synchronize()
    out, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        before()
        stream.synchronize()
        t0 = time.perf_counter()
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        out.append(a.elapsed_time(b))
    return out, wall


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("stroke_bench: no GPU", file=sys.stderr)
        return 2
    N = args.size
    rows = []

    def row(call, radius, spacing, dabs, timing):
        ms, wall = timing
        rows.append(dict(call=call, radius=radius, spacing=spacing, dabs=dabs, median_ms=statistics.median(ms),
                         min_ms=min(ms), max_ms=max(ms), host_clock_median_ms=statistics.median(wall), reps=len(ms)))
        return rows[-1]["median_ms"]

    with vr.Renderer(0) as r:
        r.generate_volume(vr.scaled_recipe(N))
        layout = r.get_option("layout")
        r.set_shader_data(*vr.reference_shader_data(16 / 9))
        s = torch.cuda.Stream()
        sh = ctypes.c_void_p(s.cuda_stream)
        ctx = r._ctx
        one = torch.from_numpy(255 - r.get_volume_box((0, 0, 0), (1, 1, 1))).cuda()
        r.update_volume(one, (0, 0, 0), stream=s)   # one texel breaks the recipe's uniform channel
        s.synchronize()
        variant = r.kernel_variant
        assert r.get_option("uniform_mask") == 0
        for radius, spacing, count in STROKES:
            # the stroke's middle dab on the volume's centre, `count` dabs along the diagonal
            first = N // 2 - spacing * (count - 1) // 2
            last = first + spacing * (count - 1)
            brush = vr.make_brush((first,) * 3, radius, vr.BRUSH_ADD, 1, VALUE, STRENGTH)
            dabs = vr.brush_line(brush, (last,) * 3, spacing)
            assert len(dabs) == count
            arr = (_lib.Brush * count)(*dabs)
            boxes = [vr.brush_box(b, (N, N, N)) for b in dabs]
            assert all(b is not None for b in boxes)
            lo = [min(o[k] for o, _ in boxes) for k in range(3)]
            hi = [max(o[k] + e[k] for o, e in boxes) for k in range(3)]
            origin, extent = tuple(lo), tuple(h - l for l, h in zip(lo, hi))
            start = r.get_volume_box(origin, extent)   # the bounding box before any edit: every path starts from it
            want = start.copy()
            for b in dabs:                             # the CPU loop, on the bounding box alone
                shifted = vr.make_brush(tuple(c - o for c, o in zip(b.centre, origin)), tuple(b.radius), b.op, b.falloff,
                                        tuple(b.value), tuple(b.strength))
                vr.brush_apply(shifted, want)
            rebuilds = len(vr.coalesce_boxes(boxes, 8))

            def stroke():
                _lib.call("vr_paint_stroke", ctx, arr, count, sh)

            def paints():
                for i in range(count):
                    _lib.call("vr_paint", ctx, ctypes.byref(arr[i]), sh)

            start_dev = torch.from_numpy(start).cuda()

            def restore():
                r.update_volume(start_dev, origin, stream=s)

            t_stroke = row("stroke", radius, spacing, count, timed(stroke, restore, s, args.warmup, args.reps))
            restore()
            stroke()
            s.synchronize()
            same = bool(np.array_equal(r.get_volume_box(origin, extent), want))
            t_paints = row("paints", radius, spacing, count, timed(paints, restore, s, args.warmup, args.reps))
            restore()
            paints()
            s.synchronize()
            same = same and bool(np.array_equal(r.get_volume_box(origin, extent), want))
            restore()
            s.synchronize()
            del start_dev
            rows.append(dict(call="agree", radius=radius, spacing=spacing, dabs=count, same_bytes=same,
                             bounding_box=list(extent), rebuild_boxes=rebuilds, paints_over_stroke=t_paints / t_stroke))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from build_id import build_id
    head = dict(tool="stroke_bench", size=N, layout=layout, variant=variant, device=torch.cuda.get_device_name(0),
                build_id=build_id(), brush="smooth ADD", value=list(VALUE), strength=list(STRENGTH),
                timing="device events around each stroke (1 call) or K paint calls, one stream", warmup=args.warmup)
    lines = [json.dumps(head)] + [json.dumps(x) for x in rows]
    print(f"# {N}^3 volume, layout {layout} ({variant}), {head['device']}, build {head['build_id']}")
    print(f"# {'call':8} {'radius':>6} {'spacing':>7} {'dabs':>5} {'median ms':>11} {'min':>10} {'max':>10} {'host clock':>11}")
    for x in rows:
        if x["call"] == "agree":
            print(f"  {'agree':8} {x['radius']:>6} {x['spacing']:>7} {x['dabs']:>5} same bytes after both paths and the CPU loop: "
                  f"{x['same_bytes']}; {x['rebuild_boxes']} rebuild boxes; paints / stroke = {x['paints_over_stroke']:.2f}")
            continue
        print(f"  {x['call']:8} {x['radius']:>6} {x['spacing']:>7} {x['dabs']:>5} {x['median_ms']:>11.4f} {x['min_ms']:>10.4f} "
              f"{x['max_ms']:>10.4f} {x['host_clock_median_ms']:>11.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(x.get("same_bytes", True) for x in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
