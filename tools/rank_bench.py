#!/usr/bin/env python3
"""Cost of a median dab (vr_rank) next to the smoothing dab of the same brush (vr_blur, same
commit launch) and to the way to make the same edit without it.

The setup of tools/morph_bench.py: a 512^3 recipe volume on the auto layout, its uniform
channel broken by one texel first; a smooth brush at the volume's centre, strength
(255, 128, 64, 255), radius 4, 16 and 64, half width 1, 2 and 3, rank VR_RANK_MEDIAN.  Per case:

  rank        vr_rank on one stream, the staging scratch reserved beforehand (no call
              allocates);
  blur        vr_blur of the same brush and half width in the same process: the same launches,
              the same commit, layout rebuild and re-arm, the other stage kernel;
  host_edit   the route without vr_rank: vr_get_volume_box of the box and its halo,
              vr_brush_rank_apply (the library's CPU statement, one thread) on it,
              vr_update_volume of the box.

Each call is timed with device events on one otherwise idle stream after warm-up calls of the
same shape (a synchronous host call's events bracket its wall time); the record gives the
median, the minimum and the maximum, and the median on the host clock.  The box is put back to
its first bytes (on the same stream, outside the events) before every timed and warm-up call
of `rank` and `blur`: a repeated median stops changing bytes after a few calls, and the commit
stores only bytes that change.  The host route takes seconds at the larger cases and is timed
`--host-reps` times without warm-up.  After the device call and the host route of a case the box
is compared: both must leave the same bytes, from the same start.  Nothing is gated: the
numbers are a record.

    python tools/rank_bench.py [--size 512] [--reps 25] [--host-reps 2] [--out FILE]
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

STRENGTH = (255, 128, 64, 255)


def timed(fn, stream, warmup, reps, before=None):
    """Milliseconds of each of `reps` calls of fn() on `stream`: (device events, host clock
    from before the call until its end event has completed).  before() runs ahead of every
    call, outside the events."""
    for _ in range(warmup):
        if before:
            before()
        fn()
    stream.synchronize()
    out, wall = [], []
    for _ in range(reps):
        if before:
            before()
            stream.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radii", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--half-widths", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("rank_bench: no GPU", file=sys.stderr)
        return 2
    N = args.size
    rows = []

    def row(call, radius, h, box, timing):
        ms_, wall = timing
        rows.append(dict(call=call, rank="median", radius=radius, half_width=h, box=list(box), median_ms=statistics.median(ms_),
                         min_ms=min(ms_), max_ms=max(ms_), host_clock_median_ms=statistics.median(wall), reps=len(ms_)))

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
        side = 2 * max(args.radii) + 1
        r.set_option("blur_scratch_kib", (4 * side ** 3 + 1023) // 1024)   # the largest case's need: no call allocates
        held = r.get_option("blur_scratch_kib")
        centre = (N // 2 + 1, N // 2 + 3, N // 2 + 5)
        for rad in args.radii:
            radius = (rad, rad, rad)
            b = vr.make_brush(centre, radius, vr.BRUSH_SET, 1, 0, STRENGTH)
            origin, extent = vr.brush_box(b, (N, N, N))
            start = r.get_volume_box(origin, extent)   # the box before any edit: every path starts from it
            d_start = torch.from_numpy(start).cuda()

            def restore():
                r.update_volume(start, origin)

            def restore_on_stream():
                r.update_volume(d_start, origin, stream=s)

            for h in args.half_widths:
                # the box and its halo, inside the volume: what the host route reads back
                lo = [max(0, o - h) for o in origin]
                hi = [min(N, o + e + h) for o, e in zip(origin, extent)]
                hext = [b_ - a_ for a_, b_ in zip(lo, hi)]
                inner = tuple(slice(o - l, o - l + e) for o, l, e in zip(origin[::-1], lo[::-1], extent[::-1]))
                local = vr.make_brush(tuple(c - l for c, l in zip(centre, lo)), radius, vr.BRUSH_SET, 1, 0, STRENGTH)

                def host_edit():
                    halo = r.get_volume_box(lo, hext)
                    # away from the volume's faces the halo holds every neighbour, so its clamped edges are never read
                    new = vr.brush_rank_apply(local, vr.RANK_MEDIAN, h, halo)[inner]
                    r.update_volume(np.ascontiguousarray(new), origin)

                row("blur", rad, h, extent, timed(lambda: _lib.call("vr_blur", ctx, ctypes.byref(b), h, sh), s,
                                                  args.warmup, args.reps, restore_on_stream))
                restore()
                row("rank", rad, h, extent,
                    timed(lambda: _lib.call("vr_rank", ctx, ctypes.byref(b), vr.RANK_MEDIAN, h, sh), s, args.warmup, args.reps,
                          restore_on_stream))
                restore()
                _lib.call("vr_rank", ctx, ctypes.byref(b), vr.RANK_MEDIAN, h, sh)
                s.synchronize()
                got = r.get_volume_box(origin, extent)
                restore()
                row("host_edit", rad, h, extent, timed(host_edit, s, 0, args.host_reps, restore))
                same = bool(np.array_equal(r.get_volume_box(origin, extent), got)) and not np.array_equal(got, start)
                restore()
                rows.append(dict(call="agree", rank="median", radius=rad, half_width=h, box=list(extent), same_bytes=same))
        assert r.get_option("blur_scratch_kib") == held, "a timed call grew the scratch"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from build_id import build_id
    head = dict(tool="rank_bench", size=N, layout=layout, variant=variant, device=torch.cuda.get_device_name(0),
                build_id=build_id(), brush="smooth", strength=list(STRENGTH), scratch_kib=held,
                timing="device events around each call, one stream; the box restored before every rank and blur call",
                warmup=args.warmup)
    lines = [json.dumps(head)] + [json.dumps(x) for x in rows]
    print(f"# {N}^3 volume, layout {layout} ({variant}), {head['device']}, build {head['build_id']}")
    print(f"# {'call':10} {'radius':>6} {'h':>2} {'box':>14} {'median ms':>11} {'min':>10} {'max':>10} {'host clock':>11}")
    for x in rows:
        if x["call"] == "agree":
            print(f"  {'agree':10} {x['radius']:>6} {x['half_width']:>2} {'':>14} vr_rank and the host route leave the "
                  f"same bytes: {x['same_bytes']}")
            continue
        box = "x".join(str(v) for v in x["box"])
        print(f"  {x['call']:10} {x['radius']:>6} {x['half_width']:>2} {box:>14} {x['median_ms']:>11.4f} "
              f"{x['min_ms']:>10.4f} {x['max_ms']:>10.4f} {x['host_clock_median_ms']:>11.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(x.get("same_bytes", True) for x in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
