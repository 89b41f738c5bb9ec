#!/usr/bin/env python3
"""Cost of a transform-paste dab (vr_stamp_affine, both filters; vr_clone_affine, both device
paths) next to vr_stamp and vr_clone of the SAME brush on the SAME volume (DESIGN.md
sec. 5.2.13).

The setup of tools/clone_bench.py: a 512^3 recipe volume on the auto layout, its uniform
channel broken by one texel first; a smooth SET brush at the volume's centre, strength
(255, 128, 64, 255), radius 4, 16 and 64.  Per radius:

  stamp                 vr_stamp of a device box of the brush's box's size, placed on the box;
  clone_direct          vr_clone with offset (2 radius + 1, 0, 0);
  clone_staged          vr_clone with offset (1, 0, 0): stage launch and commit launch;
  stamp_affine_nearest  vr_stamp_affine of the same device box turned by 30 degrees about
                        (1, 1, 2) / sqrt(6) around the brush's centre, VR_FILTER_NEAREST;
  stamp_affine_linear   the same with VR_FILTER_LINEAR: 8 dword loads per texel along a diagonal;
  stamp_affine_shift    VR_FILTER_LINEAR with a shift of half a texel and no turn: the same 8
                        loads per texel along ROWS of the source -- the difference to the line
                        above is what the diagonal costs;
  clone_affine_direct   vr_clone_affine, LINEAR, the box beside the brush's shifted by half a
                        texel onto it: one launch from the planes to the planes;
  clone_affine_staged   vr_clone_affine, LINEAR, the 30 degree turn in place: stage and commit.

The cases are timed INTERLEAVED: one call of every case per round, `reps` rounds, each call
with device events on one otherwise idle stream after warm-up rounds; the record gives the
median, the minimum and the maximum.  The box is put back to its first bytes (on the same
stream, outside the events) before every call.  Every affine case is compared once with its
host statement from the same start.  Nothing is gated: the numbers are a record.

    python tools/affine_bench.py [--size 512] [--reps 25] [--out FILE]
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
VALUE = (200, 60, 255, 10)


def rot30():
    k = np.array([1.0, 1.0, 2.0]) / np.sqrt(6.0)
    t = np.radians(30.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radii", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("affine_bench: no GPU", file=sys.stderr)
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
        centre = (N // 2 + 1 - max(args.radii), N // 2 + 3, N // 2 + 5)     # room for the source box on +x
        for rad in args.radii:
            radius = (rad, rad, rad)
            b = vr.make_brush(centre, radius, vr.BRUSH_SET, 1, VALUE, STRENGTH)
            origin, extent = vr.brush_box(b, (N, N, N))
            assert extent == (2 * rad + 1,) * 3 and origin[0] + 2 * extent[0] <= N
            start = r.get_volume_box(origin, extent)
            d_start = torch.from_numpy(start).cuda()
            beside = (origin[0] + extent[0], origin[1], origin[2])
            d_stamp = r.get_volume_box(beside, extent, stream=s)
            s.synchronize()
            h_stamp = d_stamp.cpu().numpy()
            ptr = ctypes.c_void_p(d_stamp.data_ptr())
            placement = _lib.Box(*origin, *extent)
            mid = (rad, rad, rad)                                       # the middle of the device box
            turn = {f: vr.affine_place(rot30(), mid, centre, f, vr.BORDER_CLAMP) for f in (vr.FILTER_NEAREST, vr.FILTER_LINEAR)}
            shift = vr.affine_place(np.eye(3), (rad + 0.5, rad + 0.5, rad + 0.5), centre, vr.FILTER_LINEAR, vr.BORDER_CLAMP)
            beside_half = vr.affine_place(np.eye(3), (centre[0] + extent[0] + 0.5, centre[1] + 0.5, centre[2] + 0.5), centre,
                                          vr.FILTER_LINEAR, vr.BORDER_CLAMP)
            in_place = vr.affine_place(rot30(), centre, centre, vr.FILTER_LINEAR, vr.BORDER_CLAMP)
            assert vr.affine_direct(b, beside_half, (N, N, N)) and not vr.affine_direct(b, in_place, (N, N, N))
            clone_maps = {"clone_direct": vr.make_clone_map((extent[0], 0, 0)), "clone_staged": vr.make_clone_map((1, 0, 0))}
            stamp_maps = {"stamp_affine_nearest": turn[vr.FILTER_NEAREST], "stamp_affine_linear": turn[vr.FILTER_LINEAR],
                          "stamp_affine_shift": shift}
            affine_maps = {"clone_affine_direct": beside_half, "clone_affine_staged": in_place}

            def device_call(name):
                if name == "stamp":
                    return lambda: _lib.call("vr_stamp", ctx, ctypes.byref(b), ptr, ctypes.byref(placement), sh)
                if name in clone_maps:
                    return lambda: _lib.call("vr_clone", ctx, ctypes.byref(b), ctypes.byref(clone_maps[name]), sh)
                if name in stamp_maps:
                    return lambda: _lib.call("vr_stamp_affine", ctx, ctypes.byref(b), ptr, *extent, ctypes.byref(stamp_maps[name]), sh)
                return lambda: _lib.call("vr_clone_affine", ctx, ctypes.byref(b), ctypes.byref(affine_maps[name]), sh)

            names = ["stamp", "clone_direct", "clone_staged"] + list(stamp_maps) + list(affine_maps)
            calls = {n: device_call(n) for n in names}
            times = {n: [] for n in names}
            for rnd in range(args.warmup + args.reps):
                for n in names:
                    r.update_volume(d_start, origin, stream=s)
                    s.synchronize()
                    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(s)
                    calls[n]()
                    e.record(s)
                    e.synchronize()
                    if rnd >= args.warmup:
                        times[n].append(a.elapsed_time(e))
            for n in names:
                t = times[n]
                rows.append(dict(call=n, radius=rad, box=list(extent), median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t),
                                 reps=len(t)))
            # every affine case against its host statement, from the same start
            whole = None
            for n in list(stamp_maps) + list(affine_maps):
                r.update_volume(start, origin)
                calls[n]()
                s.synchronize()
                got = r.get_volume_box(origin, extent)
                r.update_volume(start, origin)
                if n in stamp_maps:
                    m = stamp_maps[n]
                    local = vr.make_affine([list(x) for x in m.m], mid, list(m.origin), m.filter, m.border)
                    want = vr.brush_stamp_affine_apply(vr.make_brush(mid, radius, vr.BRUSH_SET, 1, VALUE, STRENGTH), h_stamp, local,
                                                       start.copy())
                else:
                    if whole is None:   # what a clone may read: the brush's box and its surroundings
                        lo = tuple(max(0, o - extent[0] - 2) for o in origin)
                        ext = tuple(min(N, o + 2 * extent[0] + 2) - l for o, l in zip(origin, lo))
                        whole = (lo, ext, r.get_volume_box(lo, ext))
                    lo, ext, block = whole
                    m = affine_maps[n]
                    local = vr.make_affine([list(x) for x in m.m], [p - l for p, l in zip(m.pivot, lo)],
                                           [o - l * 65536 for o, l in zip(m.origin, lo)], m.filter, m.border)
                    lb = vr.make_brush(tuple(c - l for c, l in zip(centre, lo)), radius, vr.BRUSH_SET, 1, VALUE, STRENGTH)
                    out = vr.brush_clone_affine_apply(lb, local, block.copy())
                    d = tuple(o - l for o, l in zip(origin, lo))
                    want = out[d[2]:d[2] + extent[2], d[1]:d[1] + extent[1], d[0]:d[0] + extent[0]]
                same = bool(np.array_equal(got, want)) and not np.array_equal(got, start)
                rows.append(dict(call="agree", route=n, radius=rad, box=list(extent), same_bytes=same))
            r.update_volume(start, origin)
        assert r.get_option("blur_scratch_kib") == held, "a timed call grew the scratch"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from build_id import build_id
    head = dict(tool="affine_bench", size=N, layout=layout, variant=variant, device=torch.cuda.get_device_name(0),
                build_id=build_id(), brush="smooth SET", strength=list(STRENGTH), scratch_kib=held,
                timing="device events around each call, one stream, the cases interleaved round by round; the box restored "
                       "before every call", warmup=args.warmup)
    lines = [json.dumps(head)] + [json.dumps(x) for x in rows]
    print(f"# {N}^3 volume, layout {layout} ({variant}), {head['device']}, build {head['build_id']}")
    print(f"# {'call':22} {'radius':>6} {'box':>14} {'median ms':>11} {'min':>10} {'max':>10}")
    for x in rows:
        if x["call"] == "agree":
            print(f"  {'agree':22} {x['radius']:>6} {'':>14} {x['route']} and its host statement leave the same bytes: {x['same_bytes']}")
            continue
        box = "x".join(str(v) for v in x["box"])
        print(f"  {x['call']:22} {x['radius']:>6} {box:>14} {x['median_ms']:>11.4f} {x['min_ms']:>10.4f} {x['max_ms']:>10.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(x.get("same_bytes", True) for x in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
