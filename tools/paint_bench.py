#!/usr/bin/env python3
"""Cost of a brush dab (vr_paint) against the ways to make the same edit without it
(DESIGN.md sec. 5.2.5).

A 512^3 recipe volume on the auto layout; a smooth SET brush of radius 4, 16 and 64 at the
volume's centre.  Per radius:

  paint        vr_paint on one stream;
  update_box   (a) vr_update_volume_device of the brush's bounding box from device memory --
               the same scatter and layout rebuild without the read-modify-write;
  host_edit    (b) the only way to make the edit before vr_paint: vr_get_volume (the whole
               volume to the host), the same blend in numpy on the box, vr_update_volume;
  get_box      (c) vr_get_volume_box of the bounding box (host, synchronous), and
  get_box_dev      vr_get_volume_box_device, against
  get_volume       vr_get_volume (once, it does not depend on the radius).

Each call is timed with device events on one otherwise idle stream after warm-up calls of the
same shape (a synchronous host call's events bracket its wall time); the table gives the
median, the minimum and the maximum, and the median on the host clock beside them.  The
uniform channel of the recipe is broken by one texel first, so every timed call is the steady
state: launches only.  After the three edit paths of a radius the volume's box is compared:
all three must leave the same bytes.  Nothing is gated: the numbers are a record.

    python tools/paint_bench.py [--size 512] [--reps 25] [--out FILE]
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

VALUE, STRENGTH = (200, 60, 255, 10), (255, 128, 64, 255)


def timed(fn, stream, warmup, reps):
    """Milliseconds of each of `reps` calls of fn() on `stream`: (device events, host clock
    from before the call until its end event has completed)."""
    for _ in range(warmup):
        fn()
    stream.synchronize()
    out, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        out.append(a.elapsed_time(b))
    return out, wall


def numpy_blend(box, origin, centre, radius):
    """The smooth SET brush of include/vr.h on a (bz, by, bx, 4) box at `origin`, in numpy."""
    bz, by, bx, _ = box.shape
    d = [np.arange(n, dtype=np.int64) + o - c for n, o, c in zip((bx, by, bz), origin, centre)]
    D2 = [np.uint64((2 * r + 1) ** 2) for r in radius]
    t = [(np.uint64(2) * np.abs(v).astype(np.uint64)) ** 2 for v in d]
    S = D2[0] * D2[1] * D2[2]
    Q = (t[0][None, None, :] * (D2[1] * D2[2]) + t[1][None, :, None] * (D2[0] * D2[2])
         + t[2][:, None, None] * (D2[0] * D2[1]))
    inside = Q <= S
    w = (np.uint64(256) - (np.uint64(256) * np.where(inside, Q, np.uint64(0))) // (S + np.uint64(1))).astype(np.int64)
    out = box.copy()
    for c in range(4):
        a = w * STRENGTH[c]
        old = box[..., c].astype(np.int64)
        new = (old * (65280 - a) + VALUE[c] * a + 32640) // 65280
        out[..., c] = np.where(inside, new, old).astype(np.uint8)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radii", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("paint_bench: no GPU", file=sys.stderr)
        return 2
    N = args.size
    rows = []

    def row(call, radius, box, timing):
        ms, wall = timing
        rows.append(dict(call=call, radius=radius, box=list(box), median_ms=statistics.median(ms), min_ms=min(ms),
                         max_ms=max(ms), host_clock_median_ms=statistics.median(wall), reps=len(ms)))

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
        whole = np.empty((N, N, N, 4), np.uint8)
        wp = whole.ctypes.data_as(ctypes.c_void_p)
        row("get_volume", 0, (N, N, N), timed(lambda: _lib.call("vr_get_volume", ctx, wp), s, args.warmup, args.reps))
        centre = (N // 2 + 1, N // 2 + 3, N // 2 + 5)
        for rad in args.radii:
            radius = (rad, rad, rad)
            b = vr.make_brush(centre, radius, vr.BRUSH_SET, 1, VALUE, STRENGTH)
            origin, extent = vr.brush_box(b, (N, N, N))
            start = r.get_volume_box(origin, extent)          # the box before any edit: every path starts from it
            want = numpy_blend(start, origin, centre, radius)

            def restore():
                r.update_volume(start, origin)

            row("paint", rad, extent, timed(lambda: _lib.call("vr_paint", ctx, ctypes.byref(b), sh), s, args.warmup,
                                            args.reps))
            restore()
            _lib.call("vr_paint", ctx, ctypes.byref(b), sh)
            s.synchronize()
            same = bool(np.array_equal(r.get_volume_box(origin, extent), want))
            dbox = torch.from_numpy(want).cuda()
            row("update_box", rad, extent,
                timed(lambda: _lib.call("vr_update_volume_device", ctx, ctypes.c_void_p(dbox.data_ptr()), *origin,
                                        *extent, sh), s, args.warmup, args.reps))
            same = same and bool(np.array_equal(r.get_volume_box(origin, extent), want))
            restore()
            x0, y0, z0 = origin
            bx, by, bz = extent

            def host_edit():
                _lib.call("vr_get_volume", ctx, wp)
                box = np.ascontiguousarray(whole[z0:z0 + bz, y0:y0 + by, x0:x0 + bx])
                new = numpy_blend(box, origin, centre, radius)
                _lib.call("vr_update_volume", ctx, new.ctypes.data_as(ctypes.c_void_p), x0, y0, z0, bx, by, bz)

            restore()
            host_edit()
            same = same and bool(np.array_equal(r.get_volume_box(origin, extent), want))
            row("host_edit", rad, extent, timed(host_edit, s, args.warmup, args.reps))
            restore()
            hbox = np.empty((bz, by, bx, 4), np.uint8)
            hp = hbox.ctypes.data_as(ctypes.c_void_p)
            row("get_box", rad, extent, timed(lambda: _lib.call("vr_get_volume_box", ctx, x0, y0, z0, bx, by, bz, hp), s,
                                              args.warmup, args.reps))
            dout = torch.empty((bz, by, bx, 4), dtype=torch.uint8, device="cuda")
            row("get_box_dev", rad, extent,
                timed(lambda: _lib.call("vr_get_volume_box_device", ctx, x0, y0, z0, bx, by, bz,
                                        ctypes.c_void_p(dout.data_ptr()), sh), s, args.warmup, args.reps))
            same = same and bool(np.array_equal(hbox, start)) and bool(np.array_equal(dout.cpu().numpy(), start))
            rows.append(dict(call="agree", radius=rad, box=list(extent), same_bytes=same))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from build_id import build_id
    head = dict(tool="paint_bench", size=N, layout=layout, variant=variant, device=torch.cuda.get_device_name(0),
                build_id=build_id(), brush="smooth SET", value=list(VALUE), strength=list(STRENGTH),
                timing="device events around each call, one stream", warmup=args.warmup)
    lines = [json.dumps(head)] + [json.dumps(x) for x in rows]
    print(f"# {N}^3 volume, layout {layout} ({variant}), {head['device']}, build {head['build_id']}")
    print(f"# {'call':12} {'radius':>6} {'box':>14} {'median ms':>11} {'min':>10} {'max':>10} {'host clock':>11}")
    for x in rows:
        if x["call"] == "agree":
            print(f"  {'agree':12} {x['radius']:>6} {'':>14} same bytes after every path: {x['same_bytes']}")
            continue
        box = "x".join(str(v) for v in x["box"])
        print(f"  {x['call']:12} {x['radius']:>6} {box:>14} {x['median_ms']:>11.4f} {x['min_ms']:>10.4f} {x['max_ms']:>10.4f} "
              f"{x['host_clock_median_ms']:>11.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(x.get("same_bytes", True) for x in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
