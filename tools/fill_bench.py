#!/usr/bin/env python3
"""Cost of a flood-fill dab (vr_fill) next to a plain dab of the same brush (vr_paint: the floor
of a brush that selects nothing) and to the route the call replaces.

A 512^3 volume on the auto layout holds three fields, one per channel, and a rule selects one:
  blob   R: a thresholded sum of sines, separate blobs of a few dozen texels across;
  snake  G: one-texel corridors along x on the rows with y and z even, joined to the next
         row every 32 texels (at alternating offsets) and to the next even plane every 32 x 32
         -- one region that winds through every tile of the box, between walls one above the
         range;
  full   B: one byte everywhere -- the whole ellipsoid is the region.
A hard SET brush at the volume's centre, strength (255, 128, 64, 0), radius 16, 64 and 255, the
seed on the field nearest the centre.  Per case:

  fill        vr_fill on one stream with a device report, the scratch reserved beforehand
              (no call allocates);
  paint       vr_paint of the same brush in the same process;
  host_route  vr_get_volume_box of the clipped box, vr_brush_fill_apply (the library's CPU
              statement, one thread) on it, vr_update_volume of the box.

Each call is timed with device events on one otherwise idle stream after warm-up calls of the
same shape; the record gives the median, the minimum and the maximum, and the median on the
host clock.  The box is put back to its first bytes (on the same stream, outside the events)
before every timed and warm-up call of `fill` and `paint`.  The host route is timed
`--host-reps` times without warm-up.  After the device call and the host route of a case the
box and the report are compared: both must agree, from the same start.  Nothing is gated: the
numbers are a record.

    python tools/fill_bench.py [--size 512] [--reps 9] [--host-reps 1] [--out FILE]
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

STRENGTH = (255, 128, 64, 0)
VALUE = (200, 60, 255, 10)
FIELDS = {"blob": 0, "snake": 1, "full": 2}


def volume(n):
    """(n, n, n, 4) uint8 with the three fields; the snake's corridor holds 100..140 and its walls 141."""
    i = np.arange(n)
    x, y, z = i[None, None, :], i[None, :, None], i[:, None, None]
    vol = np.empty((n, n, n, 4), np.uint8)
    f = np.sin(0.21 * x + 0.3) + np.sin(0.26 * y + 1.1) + np.sin(0.17 * z + 2.0)
    vol[..., 0] = np.clip(np.rint(128 + 42 * f), 0, 255)
    row = (y % 2 == 0) & (z % 2 == 0)
    turn = (z % 2 == 0) & (y % 2 == 1) & (x % 32 == np.where(y // 2 % 2 == 1, 0, 16))
    up = (z % 2 == 1) & (y % 32 == 0) & (x % 32 == 8)
    vol[..., 1] = np.where(row | turn | up, 100 + (7 * x + 3 * y + z) % 41, 141)
    vol[..., 2] = 77
    vol[..., 3] = (x + y + z) % 251
    return vol


def timed(fn, stream, warmup, reps, before=None):
    """Milliseconds of each of `reps` calls of fn() on `stream`: (device events, host clock)."""
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=1, help="0 skips the host route")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radii", type=int, nargs="+", default=[16, 64, 255])
    ap.add_argument("--fields", nargs="+", default=list(FIELDS), choices=list(FIELDS))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("fill_bench: no GPU", file=sys.stderr)
        return 2
    N = args.size
    rows = []

    def row(call, field, radius, box, timing, **extra):
        ms_, wall = timing
        rows.append(dict(call=call, field=field, radius=radius, box=list(box), median_ms=statistics.median(ms_), min_ms=min(ms_),
                         max_ms=max(ms_), host_clock_median_ms=statistics.median(wall), reps=len(ms_), **extra))

    vol = volume(N)
    with vr.Renderer(0) as r:
        r.set_volume(vol)
        layout = r.get_option("layout")
        r.set_shader_data(*vr.reference_shader_data(16 / 9))
        s = torch.cuda.Stream()
        sh = ctypes.c_void_p(s.cuda_stream)
        ctx = r._ctx
        variant = r.kernel_variant
        side = min(N, 2 * max(args.radii) + 1)
        r.set_option("blur_scratch_kib", (4 * side ** 3 + 1023) // 1024)   # the largest case's labels: no call allocates
        held = r.get_option("blur_scratch_kib")
        centre = (N // 2, N // 2, N // 2)
        report = torch.zeros(vr.FILL_REPORT_BYTES, dtype=torch.uint8, device="cuda")
        for rad in args.radii:
            radius = (rad, rad, rad)
            b = vr.make_brush(centre, radius, vr.BRUSH_SET, 0, VALUE, STRENGTH)
            origin, extent = vr.brush_box(b, (N, N, N))
            start = r.get_volume_box(origin, extent)   # the box before any edit: every path starts from it
            d_start = torch.from_numpy(start).cuda()
            local = vr.make_brush(tuple(c - o for c, o in zip(centre, origin)), radius, vr.BRUSH_SET, 0, VALUE, STRENGTH)

            def restore():
                r.update_volume(start, origin)

            def restore_on_stream():
                r.update_volume(d_start, origin, stream=s)

            row("paint", "-", rad, extent, timed(lambda: _lib.call("vr_paint", ctx, ctypes.byref(b), sh), s, args.warmup, args.reps,
                                                 restore_on_stream))
            restore()
            for field in args.fields:
                ch = FIELDS[field]
                plane = vol[..., ch]
                lo_abs, hi_abs = {"blob": (175, 255), "snake": (100, 140), "full": (77, 77)}[field]
                # the seed: the texel of the field nearest the centre within a few texels of it
                w = 20
                near = plane[centre[2] - w:centre[2] + w + 1, centre[1] - w:centre[1] + w + 1, centre[0] - w:centre[0] + w + 1]
                want = (near >= (230 if field == "blob" else lo_abs)) & (near <= hi_abs)
                cz, cy, cx = np.nonzero(want)
                k = int(np.argmin((cx - w) ** 2 + (cy - w) ** 2 + (cz - w) ** 2))
                seed = (centre[0] - w + int(cx[k]), centre[1] - w + int(cy[k]), centre[2] - w + int(cz[k]))
                sel, lo, hi = [0] * 4, [0] * 4, [0] * 4
                sel[ch], lo[ch], hi[ch] = 1, lo_abs, hi_abs
                rule = vr.make_fill_rule(seed, lo, hi, sel, 0)
                local_rule = vr.make_fill_rule(tuple(v - o for v, o in zip(seed, origin)), lo, hi, sel, 0)
                rp = ctypes.c_void_p(report.data_ptr())
                timing = timed(lambda: _lib.call("vr_fill", ctx, ctypes.byref(b), ctypes.byref(rule), rp, sh), s, args.warmup,
                               args.reps, restore_on_stream)
                rep = vr.unpack_fill_report(report)
                row("fill", field, rad, extent, timing, filled=rep.filled, passable=rep.passable)
                got = r.get_volume_box(origin, extent)
                restore()
                if args.host_reps > 0:
                    host_rep = []

                    def host_route():
                        box = r.get_volume_box(origin, extent)
                        new, hr = vr.brush_fill_apply(local, local_rule, box)
                        host_rep.append(hr)
                        r.update_volume(new, origin)

                    row("host_route", field, rad, extent, timed(host_route, s, 0, args.host_reps, restore))
                    moved = tuple(v - o for v, o in zip(rep.min, origin)), tuple(v - o for v, o in zip(rep.max, origin))
                    same = (bool(np.array_equal(r.get_volume_box(origin, extent), got)) and not np.array_equal(got, start)
                            and (host_rep[-1].filled, host_rep[-1].passable, host_rep[-1].min, host_rep[-1].max)
                            == (rep.filled, rep.passable) + moved)
                    restore()
                    rows.append(dict(call="agree", field=field, radius=rad, box=list(extent), same_bytes_and_report=same))
        assert r.get_option("blur_scratch_kib") == held, "a timed call grew the scratch"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from build_id import build_id
    head = dict(tool="fill_bench", size=N, layout=layout, variant=variant, device=torch.cuda.get_device_name(0),
                build_id=build_id(), brush="hard SET", strength=list(STRENGTH), scratch_kib=held,
                timing="device events around each call, one stream; the box restored before every fill and paint call",
                warmup=args.warmup)
    lines = [json.dumps(head)] + [json.dumps(x) for x in rows]
    print(f"# {N}^3 volume, layout {layout} ({variant}), {head['device']}, build {head['build_id']}")
    print(f"# {'call':10} {'field':>6} {'radius':>6} {'box':>14} {'median ms':>11} {'min':>10} {'max':>10} {'host clock':>11} {'filled':>10} {'passable':>10}")
    for x in rows:
        if x["call"] == "agree":
            print(f"  {'agree':10} {x['field']:>6} {x['radius']:>6} vr_fill and the host route leave the same bytes and report: "
                  f"{x['same_bytes_and_report']}")
            continue
        box = "x".join(str(v) for v in x["box"])
        print(f"  {x['call']:10} {x['field']:>6} {x['radius']:>6} {box:>14} {x['median_ms']:>11.4f} {x['min_ms']:>10.4f} "
              f"{x['max_ms']:>10.4f} {x['host_clock_median_ms']:>11.4f} {x.get('filled', ''):>10} {x.get('passable', ''):>10}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(x.get("same_bytes_and_report", True) for x in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
