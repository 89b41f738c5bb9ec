#!/usr/bin/env python3
"""Cost of a clone dab (vr_clone, both device paths) and of a stamp dab (vr_stamp) next to the
constant-value dab of the same brush (vr_paint, same build) and to the way to make the same
edit without them.

The setup of tools/morph_bench.py: a 512^3 recipe volume on the auto layout, its uniform
channel broken by one texel first; a smooth SET brush at the volume's centre, strength
(255, 128, 64, 255), radius 4, 16 and 64.  Per radius:

  paint         vr_paint of the brush: the launch the other three are shaped after;
  clone_direct  vr_clone with offset (2 radius + 1, 0, 0): the source box lies beside the
                brush's box, one launch from the planes to the planes;
  clone_staged  vr_clone with offset (1, 0, 0), a push: the stage launch to the staging
                scratch (reserved beforehand: no call allocates) and the blur's commit launch;
  stamp         vr_stamp of a device box of the brush's box's size (cut from the volume beside
                it with vr_get_volume_box_device beforehand), placed on the brush's box;
  host_clone_direct, host_clone_staged, host_stamp
                the route without them: vr_get_volume_box of what the edit reads and writes
                (for a clone the bounding box of the brush's box and its source), the host
                statement (vr_brush_clone_apply / vr_brush_stamp_apply) on it, vr_update_volume
                of the brush's box.

Each call is timed with device events on one otherwise idle stream after warm-up calls of the
same shape (a synchronous host call's events bracket its wall time); the record gives the
median, the minimum and the maximum, and the median on the host clock.  The box is put back
to its first bytes (on the same stream, outside the events) before every timed and warm-up
call, so that every call changes the same bytes.  After the device call and the host route of
a case the box is compared: both must leave the same bytes, from the same start.  Nothing is
gated: the numbers are a record.

    python tools/clone_bench.py [--size 512] [--reps 25] [--out FILE]
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
VALUE = (200, 60, 255, 10)


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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radii", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("clone_bench: no GPU", file=sys.stderr)
        return 2
    N = args.size
    rows = []

    def row(call, radius, box, timing):
        ms_, wall = timing
        rows.append(dict(call=call, radius=radius, box=list(box), median_ms=statistics.median(ms_), min_ms=min(ms_),
                         max_ms=max(ms_), host_clock_median_ms=statistics.median(wall), reps=len(ms_)))

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
        centre = (N // 2 + 1 - max(args.radii), N // 2 + 3, N // 2 + 5)     # room for the source box on +x
        for rad in args.radii:
            radius = (rad, rad, rad)
            b = vr.make_brush(centre, radius, vr.BRUSH_SET, 1, VALUE, STRENGTH)
            origin, extent = vr.brush_box(b, (N, N, N))
            assert extent == (2 * rad + 1,) * 3 and origin[0] + 2 * extent[0] <= N
            start = r.get_volume_box(origin, extent)   # the box before any edit: every path starts from it
            d_start = torch.from_numpy(start).cuda()
            beside = (origin[0] + extent[0], origin[1], origin[2])
            d_stamp = r.get_volume_box(beside, extent, stream=s)   # what the direct clone reads, as a device box
            s.synchronize()
            h_stamp = d_stamp.cpu().numpy()
            placement = _lib.Box(*origin, *extent)
            maps = {"clone_direct": vr.make_clone_map((extent[0], 0, 0)), "clone_staged": vr.make_clone_map((1, 0, 0))}

            def restore():
                r.update_volume(start, origin)

            def restore_on_stream():
                r.update_volume(d_start, origin, stream=s)

            def device_call(name):
                if name == "paint":
                    return lambda: _lib.call("vr_paint", ctx, ctypes.byref(b), sh)
                if name == "stamp":
                    return lambda: _lib.call("vr_stamp", ctx, ctypes.byref(b), ctypes.c_void_p(d_stamp.data_ptr()),
                                             ctypes.byref(placement), sh)
                return lambda: _lib.call("vr_clone", ctx, ctypes.byref(b), ctypes.byref(maps[name]), sh)

            def host_route(name):
                if name == "stamp":
                    def edit():
                        box = r.get_volume_box(origin, extent)
                        local = vr.make_brush((rad, rad, rad), radius, vr.BRUSH_SET, 1, VALUE, STRENGTH)
                        vr.brush_stamp_apply(local, h_stamp, (0, 0, 0), box)
                        r.update_volume(box, origin)
                    return edit
                m = maps[name]
                reach = max(int(m.offset[0]), 0)   # the source lies on +x: read the box and its source in one box

                def edit():
                    both = r.get_volume_box(origin, (extent[0] + reach, extent[1], extent[2]))
                    local = vr.make_brush((rad, rad, rad), radius, vr.BRUSH_SET, 1, VALUE, STRENGTH)
                    vr.brush_clone_apply(local, m, both)
                    r.update_volume(np.ascontiguousarray(both[:, :, :extent[0]]), origin)
                return edit

            for name in ("paint", "clone_direct", "clone_staged", "stamp"):
                call = device_call(name)
                row(name, rad, extent, timed(call, s, args.warmup, args.reps, restore_on_stream))
                restore()
                if name == "paint":
                    continue
                call()
                s.synchronize()
                got = r.get_volume_box(origin, extent)
                restore()
                edit = host_route(name)
                edit()
                same = bool(np.array_equal(r.get_volume_box(origin, extent), got)) and not np.array_equal(got, start)
                restore()
                row("host_" + name, rad, extent, timed(edit, s, args.warmup, args.reps, restore))
                restore()
                rows.append(dict(call="agree", route=name, radius=rad, box=list(extent), same_bytes=same))
        assert r.get_option("blur_scratch_kib") == held, "a timed call grew the scratch"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from build_id import build_id
    head = dict(tool="clone_bench", size=N, layout=layout, variant=variant, device=torch.cuda.get_device_name(0),
                build_id=build_id(), brush="smooth SET", strength=list(STRENGTH), scratch_kib=held,
                timing="device events around each call, one stream; the box restored before every call",
                warmup=args.warmup)
    lines = [json.dumps(head)] + [json.dumps(x) for x in rows]
    print(f"# {N}^3 volume, layout {layout} ({variant}), {head['device']}, build {head['build_id']}")
    print(f"# {'call':18} {'radius':>6} {'box':>14} {'median ms':>11} {'min':>10} {'max':>10} {'host clock':>11}")
    for x in rows:
        if x["call"] == "agree":
            print(f"  {'agree':18} {x['radius']:>6} {'':>14} {x['route']} and its host route leave the same bytes: {x['same_bytes']}")
            continue
        box = "x".join(str(v) for v in x["box"])
        print(f"  {x['call']:18} {x['radius']:>6} {box:>14} {x['median_ms']:>11.4f} {x['min_ms']:>10.4f} {x['max_ms']:>10.4f} "
              f"{x['host_clock_median_ms']:>11.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(x.get("same_bytes", True) for x in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
