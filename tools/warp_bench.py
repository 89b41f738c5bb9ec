#!/usr/bin/env python3
"""Cost of a liquify dab (vr_warp) through both paths of its stage kernel, next to the staged
vr_clone_affine of the SAME brush and map on the SAME volume.

The setup of tools/affine_bench.py: a 512^3 recipe volume on the auto layout, its uniform
channel broken by one texel first; a smooth SET brush at the volume's centre, strength
(255, 128, 64, 255), radius 8, 32 and 128; VR_FILTER_LINEAR, VR_BORDER_CLAMP.  Per radius and
map (a push by 3 texels along x, a twirl by 20 degrees about z, a pinch to 0.8):

  warp_lds1      vr_warp with option warp_lds = 1: a tile whose footprint fits stages it in LDS;
  warp_lds0      vr_warp with warp_lds = 0: every tile gathers its corners from the planes;
  clone_affine   vr_clone_affine, staged, of the same brush and map: the nearest capability the
                 library had before vr_warp (a wave per box row, eight byte gathers per texel and
                 channel) -- it computes a different thing (a cross-fade), at the same traffic.

The cases are timed INTERLEAVED: one call of every case per round, `reps` rounds, each call
with device events on one otherwise idle stream after warm-up rounds; the record gives the
median, the minimum and the maximum.  The box is put back to its first bytes (on the same
stream, outside the events) before every call.  Both warp paths are compared once per shape
with each other and, up to radius 32, with the host statement.  Nothing is gated: the numbers
are a record.

    python tools/warp_bench.py [--size 512] [--reps 15] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import volumetricrenderer_amd as vr  # noqa: E402
from volumetricrenderer_amd import _lib  # noqa: E402

STRENGTH = (255, 128, 64, 255)


def rot_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radii", type=int, nargs="+", default=[8, 32, 128])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("warp_bench: no GPU", file=sys.stderr)
        return 2
    N = args.size
    rows = []
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
        side = 2 * max(args.radii) + 1
        r.set_option("blur_scratch_kib", (4 * side ** 3 + 1023) // 1024)   # the largest case's need: no call allocates
        held = r.get_option("blur_scratch_kib")
        centre = (N // 2 + 1, N // 2 + 3, N // 2 + 5)
        L, C = vr.FILTER_LINEAR, vr.BORDER_CLAMP
        maps = {"push3": vr.warp_push(centre, (3 << 16, 0, 0), L, C),
                "twirl20": vr.affine_place(rot_z(20.0), centre, centre, L, C),
                "pinch08": vr.affine_place(np.eye(3) * 0.8, centre, centre, L, C)}
        for rad in args.radii:
            radius = (rad, rad, rad)
            b = vr.make_brush(centre, radius, vr.BRUSH_SET, 1, 0, STRENGTH)
            origin, extent = vr.brush_box(b, (N, N, N))
            assert extent == (2 * rad + 1,) * 3
            d_start = r.get_volume_box(origin, extent, stream=s)
            s.synchronize()
            start = d_start.cpu().numpy()
            for mname, m in maps.items():
                assert not vr.affine_direct(b, m, (N, N, N))

                def warp():
                    _lib.call("vr_warp", ctx, ctypes.byref(b), ctypes.byref(m), sh)

                calls = {"warp_lds1": warp, "warp_lds0": warp,
                         "clone_affine": lambda: _lib.call("vr_clone_affine", ctx, ctypes.byref(b), ctypes.byref(m), sh)}
                lds = {"warp_lds1": 1, "warp_lds0": 0, "clone_affine": 1}   # set outside the events
                times = {n: [] for n in calls}
                for rnd in range(args.warmup + args.reps):
                    for n in calls:
                        r.update_volume(d_start, origin, stream=s)
                        r.set_option("warp_lds", lds[n])
                        s.synchronize()
                        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(s)
                        calls[n]()
                        e.record(s)
                        e.synchronize()
                        if rnd >= args.warmup:
                            times[n].append(a.elapsed_time(e))
                for n in calls:
                    t = times[n]
                    rows.append(dict(call=n, map=mname, radius=rad, box=list(extent), median_ms=statistics.median(t), min_ms=min(t),
                                     max_ms=max(t), reps=len(t)))
                # both paths from the same start: the same bytes, and (small boxes) the host statement's
                got = {}
                for n in ("warp_lds1", "warp_lds0"):
                    r.update_volume(d_start, origin, stream=s)
                    r.set_option("warp_lds", lds[n])
                    calls[n]()
                    s.synchronize()
                    got[n] = r.get_volume_box(origin, extent)
                r.update_volume(d_start, origin, stream=s)
                s.synchronize()
                same = bool(np.array_equal(got["warp_lds1"], got["warp_lds0"])) and not np.array_equal(got["warp_lds1"], start)
                host = None
                if rad <= 32:   # what the warp may read: the brush's box and a margin wider than any displacement
                    pad = rad // 2 + 6
                    lo = tuple(o - pad for o in origin)
                    ext = tuple(x + 2 * pad for x in extent)
                    block = r.get_volume_box(lo, ext)
                    local = vr.make_affine([list(x) for x in m.m], [p - l for p, l in zip(m.pivot, lo)],
                                           [o - l * 65536 for o, l in zip(m.origin, lo)], m.filter, m.border)
                    lb = vr.make_brush(tuple(c - l for c, l in zip(centre, lo)), radius, vr.BRUSH_SET, 1, 0, STRENGTH)
                    out = vr.brush_warp_apply(lb, local, block.copy())
                    want = out[pad:pad + extent[2], pad:pad + extent[1], pad:pad + extent[0]]
                    host = bool(np.array_equal(got["warp_lds1"], want))
                rows.append(dict(call="agree", map=mname, radius=rad, box=list(extent), same_bytes=same, host_statement=host))
        r.set_option("warp_lds", 1)
        assert r.get_option("blur_scratch_kib") == held, "a timed call grew the scratch"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from build_id import build_id
    head = dict(tool="warp_bench", size=N, layout=layout, variant=variant, device=torch.cuda.get_device_name(0),
                build_id=build_id(), brush="smooth SET, LINEAR, CLAMP", strength=list(STRENGTH), scratch_kib=held,
                timing="device events around each call, one stream, the cases interleaved round by round; the box restored "
                       "before every call", warmup=args.warmup)
    lines = [json.dumps(head)] + [json.dumps(x) for x in rows]
    print(f"# {N}^3 volume, layout {layout} ({variant}), {head['device']}, build {head['build_id']}")
    print(f"# {'call':14} {'map':>8} {'radius':>6} {'box':>12} {'median ms':>11} {'min':>10} {'max':>10}")
    for x in rows:
        if x["call"] == "agree":
            print(f"  {'agree':14} {x['map']:>8} {x['radius']:>6} both paths leave the same bytes: {x['same_bytes']}; "
                  f"the host statement's: {x['host_statement']}")
            continue
        box = "x".join(str(v) for v in x["box"])
        print(f"  {x['call']:14} {x['map']:>8} {x['radius']:>6} {box:>12} {x['median_ms']:>11.4f} {x['min_ms']:>10.4f} {x['max_ms']:>10.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(x.get("same_bytes", True) and x.get("host_statement") is not False for x in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
