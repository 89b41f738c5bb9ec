#!/usr/bin/env python3
"""Cost of the statistics under a brush (vr_brush_stats, vr_box_stats) against their floor
and against the way to get the same numbers without them.

The setup of tools/blur_bench.py: a 512^3 recipe volume on the auto layout; a brush at the
volume's centre, all four channels selected, radius 4, 16 and 64, hard and smooth; and
vr_box_stats of the whole volume.  Every case runs twice: on the recipe volume as generated,
whose G channel is constant (every wave of k_stats takes the one-atomic path for G), and
after one texel has broken G (the record's "g" is "constant" or "broken").  Per case:

  stats       vr_brush_stats (or vr_box_stats) into a device buffer on one stream;
  unpack      vr_get_volume_box_device of the brush's clipped box (of the whole volume for
              the box case) into a device buffer: it reads the same plane bytes and writes
              four bytes per texel, the floor for what a pass over the box can cost;
  host_route  the route without the call: vr_get_volume_box of the box to the host, then
              np.bincount per channel (for a brush: over the texels paint_spec's mask
              selects, with its weights).  Skipped for the whole volume above --host-max
              texels; the record then says so.

Each call is timed with device events on one otherwise idle stream after warm-up calls of the
same shape (a synchronous host call's events bracket its wall time); the record gives the
median, the minimum and the maximum, and the median on the host clock.  After the timed calls
of a case the device result is compared with the host route's: every field must agree.
Nothing is gated: the numbers are a record.

    python tools/stats_bench.py [--size 512] [--reps 25] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import paint_spec as ps  # noqa: E402
import volumetricrenderer_amd as vr  # noqa: E402
from volumetricrenderer_amd import _lib  # noqa: E402

FULL = (255, 255, 255, 255)


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


def host_stats(box, centre_local, radius, falloff):
    """count, weight, wsum, hist of a read-back box (bz, by, bx, 4) in numpy; centre_local = None: every texel."""
    if centre_local is None:
        sel = box.reshape(-1, 4)
        w = None
    else:
        inside, wt = ps.spec_weights(box.shape[:3], centre_local, radius, falloff)
        sel, w = box[inside], wt[inside]
    n = len(sel)
    hist = np.stack([np.bincount(sel[:, c], minlength=256) for c in range(4)])
    if w is None:
        weight, wsum = 256 * n, 256 * (hist * np.arange(256)).sum(axis=1)
    else:
        weight, wsum = int(w.sum()), np.array([int((sel[:, c].astype(np.int64) * w).sum()) for c in range(4)])
    return n, int(weight), np.asarray(wsum, np.int64), hist.astype(np.int64)


def agree(st, host):
    n, weight, wsum, hist = host
    return bool(st.count == n and st.weight == weight and np.array_equal(st.wsum.astype(np.int64), wsum)
                and np.array_equal(st.hist.astype(np.int64), hist))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radii", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--host-reps", type=int, default=5, help="timed host-route calls of a box above 1e6 texels")
    ap.add_argument("--host-max", type=int, default=1 << 28, help="largest box (texels) the host route is run on")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("stats_bench: no GPU", file=sys.stderr)
        return 2
    N = args.size
    rows = []

    def row(g, call, what, falloff, box, timing):
        ms, wall = timing
        rows.append(dict(g=g, call=call, case=what, falloff=falloff, box=list(box), median_ms=statistics.median(ms),
                         min_ms=min(ms), max_ms=max(ms), host_clock_median_ms=statistics.median(wall), reps=len(ms)))

    with vr.Renderer(0) as r:
        r.generate_volume(vr.scaled_recipe(N))
        layout = r.get_option("layout")
        r.set_shader_data(*vr.reference_shader_data(16 / 9))
        s = torch.cuda.Stream()
        sh = ctypes.c_void_p(s.cuda_stream)
        ctx = r._ctx
        variant = r.kernel_variant
        d_stats = torch.empty(vr.VOLUME_STATS_BYTES, dtype=torch.uint8, device="cuda")
        sp = ctypes.c_void_p(d_stats.data_ptr())
        centre = (N // 2 + 1, N // 2 + 3, N // 2 + 5)
        d_box = torch.empty(4 * N ** 3, dtype=torch.uint8, device="cuda")   # room for the largest box: the volume
        bp = ctypes.c_void_p(d_box.data_ptr())
        for g in ("constant", "broken"):
            if g == "broken":
                one = torch.from_numpy(255 - r.get_volume_box((0, 0, 0), (1, 1, 1))).cuda()
                r.update_volume(one, (0, 0, 0), stream=s)   # one texel breaks the recipe's uniform channel
                s.synchronize()
                assert r.get_option("uniform_mask") == 0
            else:
                assert r.get_option("uniform_mask") & 2, "the recipe's G is not uniform"
            for rad in args.radii:
                radius = (rad, rad, rad)
                for falloff in (0, 1):
                    b = vr.make_brush(centre, radius, vr.BRUSH_SET, falloff, 0, FULL)
                    origin, extent = vr.brush_box(b, (N, N, N))
                    local = tuple(c - o for c, o in zip(centre, origin))
                    what = f"brush r={rad}"
                    row(g, "stats", what, falloff, extent,
                        timed(lambda: _lib.call("vr_brush_stats", ctx, ctypes.byref(b), sp, sh), s, args.warmup, args.reps))
                    st = vr.unpack_stats(d_stats)
                    if falloff == 0:   # the floor and the box do not depend on the falloff
                        row(g, "unpack", what, falloff, extent,
                            timed(lambda: _lib.call("vr_get_volume_box_device", ctx, *origin, *extent, bp, sh), s,
                                  args.warmup, args.reps))
                    texels = extent[0] * extent[1] * extent[2]
                    reps = args.reps if texels <= 10 ** 6 else args.host_reps
                    host = []

                    def host_route():
                        host[:] = [host_stats(r.get_volume_box(origin, extent), local, radius, falloff)]

                    row(g, "host_route", what, falloff, extent, timed(host_route, s, 1, reps))
                    rows.append(dict(g=g, call="agree", case=what, falloff=falloff, box=list(extent), same=agree(st, host[0])))
            # the whole volume
            whole = ((0, 0, 0), (N, N, N))
            row(g, "stats", "box whole", 0, whole[1],
                timed(lambda: _lib.call("vr_box_stats", ctx, *whole[0], *whole[1], 0xF, sp, sh), s, args.warmup, args.reps))
            st = vr.unpack_stats(d_stats)
            row(g, "unpack", "box whole", 0, whole[1],
                timed(lambda: _lib.call("vr_get_volume_box_device", ctx, *whole[0], *whole[1], bp, sh), s, args.warmup,
                      args.reps))
            if N ** 3 <= args.host_max:
                host = []

                def host_whole():
                    host[:] = [host_stats(r.get_volume_box(*whole), None, None, 0)]

                row(g, "host_route", "box whole", 0, whole[1], timed(host_whole, s, 0, max(1, args.host_reps // 2)))
                rows.append(dict(g=g, call="agree", case="box whole", falloff=0, box=list(whole[1]), same=agree(st, host[0])))
            else:
                rows.append(dict(g=g, call="host_route", case="box whole", skipped=f"{N}^3 texels exceed --host-max"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from build_id import build_id
    head = dict(tool="stats_bench", size=N, layout=layout, variant=variant, device=torch.cuda.get_device_name(0),
                build_id=build_id(), channels="all four", centre=list(centre),
                timing="device events around each call, one stream", warmup=args.warmup)
    lines = [json.dumps(head)] + [json.dumps(x) for x in rows]
    print(f"# {N}^3 volume, layout {layout} ({variant}), {head['device']}, build {head['build_id']}")
    print(f"# {'G':8} {'call':10} {'case':12} {'edge':>6} {'box':>14} {'median ms':>11} {'min':>10} {'max':>10} {'host clock':>11}")
    for x in rows:
        if x["call"] == "agree":
            print(f"  {x['g']:8} {'agree':10} {x['case']:12} {'':>6} {'':>14} device and host route agree in every field: {x['same']}")
            continue
        if "skipped" in x:
            print(f"  {x['g']:8} {x['call']:10} {x['case']:12} skipped: {x['skipped']}")
            continue
        box = "x".join(str(v) for v in x["box"])
        print(f"  {x['g']:8} {x['call']:10} {x['case']:12} {'smooth' if x['falloff'] else 'hard':>6} {box:>14} {x['median_ms']:>11.4f} "
              f"{x['min_ms']:>10.4f} {x['max_ms']:>10.4f} {x['host_clock_median_ms']:>11.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(x.get("same", True) for x in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
