#!/usr/bin/env python3
"""Cost of a lookup-table dab (vr_remap with a host table, vr_remap_device with a device
table), of a table built from stats on the device (vr_stats_lut_device) and of the whole
device chain stats -> table -> remap, next to the constant-value dab of the same brush
(vr_paint, same build), to the staged clone of the same box and to the way to make the same
edit without them.

The setup of tools/clone_bench.py: a 512^3 recipe volume on the auto layout, its uniform
channel broken by one texel first; a smooth SET brush at the volume's centre, strength
(255, 128, 64, 255), radius 4, 16 and 64.  Per radius:

  paint          vr_paint of the brush: the yardstick, the launch the remap is shaped after;
  remap          vr_remap with a host table (a fixed-seed permutation per channel): the 1024
                 bytes travel in the kernel's arguments;
  remap_device   vr_remap_device with the same table in device memory;
  clone_staged   vr_clone with offset (1, 0, 0), a push, of the same box (scratch reserved);
  stats_lut      vr_stats_lut_device alone (VR_LUT_EQUALIZE of the brush's stats, all channels);
  chain          vr_brush_stats + vr_stats_lut_device + vr_remap_device, back to back;
  host_remap     the route without them: vr_get_volume_box of the brush's box, the host
                 statement (vr_brush_remap_apply) on it, vr_update_volume of the box.

Each call is timed with device events on one otherwise idle stream after warm-up calls of the
same shape (a synchronous host call's events bracket its wall time); the record gives the
median, the minimum and the maximum, and the median on the host clock.  The box is put back
to its first bytes (on the same stream, outside the events) before every timed and warm-up
call, so that every call changes the same bytes.  After the device calls and the host route
the box is compared: all must leave the same bytes, from the same start.  Nothing is gated:
the numbers are a record.

    python tools/remap_bench.py [--size 512] [--reps 25] [--out FILE]
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
    ap.add_argument("--out", default="profiles/paint/remap_bench.jsonl")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("remap_bench: no GPU", file=sys.stderr)
        return 2
    N = args.size
    rows = []
    rng = np.random.default_rng(20241020)
    perm = np.stack([rng.permutation(256) for _ in range(4)]).astype(np.uint8)

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
        r.set_option("blur_scratch_kib", (4 * side ** 3 + 1023) // 1024)   # the staged clone's need: no call allocates
        held = r.get_option("blur_scratch_kib")
        centre = (N // 2 + 1, N // 2 + 3, N // 2 + 5)
        h_lut = _lib.Lut()
        ctypes.memmove(ctypes.byref(h_lut), perm.ctypes.data, vr.LUT_BYTES)
        d_lut = torch.from_numpy(perm).cuda()
        d_eq = torch.zeros((4, 256), dtype=torch.uint8, device="cuda")
        d_stats = torch.zeros(vr.VOLUME_STATS_BYTES, dtype=torch.uint8, device="cuda")
        push = vr.make_clone_map((1, 0, 0))
        for rad in args.radii:
            radius = (rad, rad, rad)
            b = vr.make_brush(centre, radius, vr.BRUSH_SET, 1, VALUE, STRENGTH)
            origin, extent = vr.brush_box(b, (N, N, N))
            assert extent == (2 * rad + 1,) * 3
            start = r.get_volume_box(origin, extent)   # the box before any edit: every path starts from it
            d_start = torch.from_numpy(start).cuda()

            def restore():
                r.update_volume(start, origin)

            def restore_on_stream():
                r.update_volume(d_start, origin, stream=s)

            def stats():
                _lib.call("vr_brush_stats", ctx, ctypes.byref(b), ctypes.c_void_p(d_stats.data_ptr()), sh)

            def table():
                _lib.call("vr_stats_lut_device", ctx, ctypes.c_void_p(d_stats.data_ptr()), vr.LUT_EQUALIZE, 15,
                          ctypes.c_void_p(d_eq.data_ptr()), sh)

            def chain():
                stats()
                table()
                _lib.call("vr_remap_device", ctx, ctypes.byref(b), ctypes.c_void_p(d_eq.data_ptr()), sh)

            calls = {
                "paint": lambda: _lib.call("vr_paint", ctx, ctypes.byref(b), sh),
                "remap": lambda: _lib.call("vr_remap", ctx, ctypes.byref(b), ctypes.byref(h_lut), sh),
                "remap_device": lambda: _lib.call("vr_remap_device", ctx, ctypes.byref(b), ctypes.c_void_p(d_lut.data_ptr()), sh),
                "clone_staged": lambda: _lib.call("vr_clone", ctx, ctypes.byref(b), ctypes.byref(push), sh),
                "chain": chain,
            }

            def host_remap():
                box = r.get_volume_box(origin, extent)
                local = vr.make_brush((rad, rad, rad), radius, vr.BRUSH_SET, 1, VALUE, STRENGTH)
                vr.brush_remap_apply(local, perm, box)
                r.update_volume(box, origin)

            got = {}
            for name, call in calls.items():
                row(name, rad, extent, timed(call, s, args.warmup, args.reps, restore_on_stream))
                restore()
                call()
                s.synchronize()
                got[name] = r.get_volume_box(origin, extent)
                restore()
            restore()
            stats()
            s.synchronize()
            row("stats_lut", rad, extent, timed(table, s, args.warmup, args.reps))
            host_remap()
            got["host_remap"] = r.get_volume_box(origin, extent)
            restore()
            row("host_remap", rad, extent, timed(host_remap, s, args.warmup, args.reps, restore))
            restore()
            # the chain's bytes: the host statement with the host's table from the host's stats
            st = r.brush_stats(centre, radius, 1, STRENGTH)
            eq = vr.stats_lut(st, vr.LUT_EQUALIZE)
            want_chain = start.copy()
            vr.brush_remap_apply(vr.make_brush((rad, rad, rad), radius, vr.BRUSH_SET, 1, VALUE, STRENGTH), eq, want_chain)
            same = (bool(np.array_equal(got["remap"], got["host_remap"])) and bool(np.array_equal(got["remap_device"], got["host_remap"]))
                    and not np.array_equal(got["remap"], start))
            rows.append(dict(call="agree", route="remap, remap_device and host_remap", radius=rad, box=list(extent), same_bytes=same))
            rows.append(dict(call="agree", route="chain and the host chain", radius=rad, box=list(extent),
                             same_bytes=bool(np.array_equal(got["chain"], want_chain))))
        assert r.get_option("blur_scratch_kib") == held, "a timed call grew the scratch"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from build_id import build_id
    head = dict(tool="remap_bench", size=N, layout=layout, variant=variant, device=torch.cuda.get_device_name(0),
                build_id=build_id(), brush="smooth SET", strength=list(STRENGTH), table="a fixed-seed permutation per channel",
                scratch_kib=held, timing="device events around each call, one stream; the box restored before every call",
                warmup=args.warmup)
    lines = [json.dumps(head)] + [json.dumps(x) for x in rows]
    print(f"# {N}^3 volume, layout {layout} ({variant}), {head['device']}, build {head['build_id']}")
    print(f"# {'call':18} {'radius':>6} {'box':>14} {'median ms':>11} {'min':>10} {'max':>10} {'host clock':>11}")
    for x in rows:
        if x["call"] == "agree":
            print(f"  {'agree':18} {x['radius']:>6} {'':>14} {x['route']} leave the same bytes: {x['same_bytes']}")
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
