#!/usr/bin/env python3
"""The edit loop `update box -> re-render its footprint` against `update box ->
re-render the frame`.

A 512^3 recipe volume on the auto layout at 1920 x 1080 x 128 steps with the
reference camera; texel boxes of 16^3, 64^3, 128^3 and 256^3, each at an
aligned and an odd origin.  Per box, in one process and on one stream:

* the footprint (vr_update_footprint) and its area as a share of the frame;
* device-event time of vr_update_volume_device + vr_render_rect(footprint);
* the same for vr_update_volume_device + vr_render of the whole frame.

Each pair is timed after warm-up calls of the same shape; the record keeps the
median, the minimum and the maximum.  Two passes, as tools/volume_update_bench.py:
with the recipe's uniform G still held (every update re-arms the read-back that
the next vr_render waits for on the host; vr_render_rect never waits) and after
one texel has broken it.  Also timed alone: vr_render of the frame, and
vr_render_rect of one 8 x 8 tile under the projected box centre -- the floor
that the longest ray of an underfilled launch sets.

No ratio is required: the tool prints, per box, whether the rectangle path was
faster, and always exits 0 when it ran.

    python tools/rect_render_bench.py [--size 512] [--reps 25] [--out FILE]
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

import torch  # noqa: E402

import volumetricrenderer_amd as vr  # noqa: E402
from volumetricrenderer_amd import _lib  # noqa: E402
from volume_update_bench import timed  # noqa: E402


def summary(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("rect_render_bench: no GPU", file=sys.stderr)
        return 2
    N, W, H = args.size, args.width, args.height
    fmt = vr.FMT_RGBA8_UNORM
    rows = []
    with vr.Renderer(0) as r:
        r.generate_volume(vr.scaled_recipe(N))
        layout = r.get_option("layout")
        osd, gsd = vr.reference_shader_data(W / H)
        r.set_shader_data(osd, gsd)
        r.set_march(vr.march_defaults(max_steps=args.steps))
        variant = r.kernel_variant
        vol = torch.from_numpy(r.get_volume()).cuda()
        frame = r.alloc_target(W, H, fmt)
        s = torch.cuda.Stream()
        sh = ctypes.c_void_p(s.cuda_stream)
        ctx = r._ctx
        target = _lib.Target(width=W, height=H, format=fmt, band_rows=0, band_stride=1, band_first=0,
                             pixels=frame.data_ptr(), row_pitch=frame.stride(0), step_counter=None)
        odd = (N // 4 + 1, N // 4 + 3, N // 4 + 5)
        cases = []
        for e in (16, 64, 128, 256):
            for tag, o in (("aligned", (N // 4,) * 3), ("odd", odd)):
                if max(o) + e > N:
                    continue
                box = vol[o[2]:o[2] + e, o[1]:o[1] + e, o[0]:o[0] + e].contiguous()
                cases.append((e, tag, o, box))
        torch.cuda.synchronize()

        def update(o, e, box):
            _lib.call("vr_update_volume_device", ctx, ctypes.c_void_p(box.data_ptr()), *o, e, e, e, sh)

        def render():
            _lib.call("vr_render", ctx, ctypes.byref(target), sh)

        def render_rect(rect):
            _lib.call("vr_render_rect", ctx, ctypes.byref(target), ctypes.byref(rect), sh)

        for held in (True, False):
            r.set_volume_device(vol, stream=s)
            if not held:   # one texel breaks the uniform channel(s); resolve it before timing
                t = vol[:1, :1, :1].clone()
                t[..., :] = 255 - t
                r.update_volume(t, (0, 0, 0), stream=s)
                s.synchronize()
            mask = r.get_option("uniform_mask")
            whole = summary(timed(render, s, args.warmup, args.reps))
            rows.append(dict(call="render", uniform_mask=mask, rect=[0, 0, W, H], frame_share=1.0, **whole))
            cx, cy = W // 2 & ~7, H // 2 & ~7
            tile = _lib.Rect(cx, cy, 8, 8)
            rows.append(dict(call="render_rect_one_tile", uniform_mask=mask, rect=[cx, cy, 8, 8],
                             frame_share=64 / (W * H), **summary(timed(lambda: render_rect(tile), s, args.warmup,
                                                                       args.reps))))
            for e, tag, o, box in cases:
                fp = _lib.Rect()
                _lib.call("vr_update_footprint", ctx, W, H, *o, e, e, e, ctypes.byref(fp))
                share = fp.width * fp.height / (W * H)

                def edit_rect():
                    update(o, e, box)
                    render_rect(fp)

                def edit_frame():
                    update(o, e, box)
                    render()

                a = summary(timed(edit_rect, s, args.warmup, args.reps))
                b = summary(timed(edit_frame, s, args.warmup, args.reps))
                rows.append(dict(call="edit", box=e, origin=list(o), align=tag, uniform_mask=mask,
                                 rect=[fp.x, fp.y, fp.width, fp.height], frame_share=share,
                                 rect_path=a, frame_path=b, rect_faster=a["median_ms"] < b["median_ms"]))
        s.synchronize()
    head = dict(tool="rect_render_bench", size=N, width=W, height=H, steps=args.steps, format=fmt, layout=layout,
                variant=variant, device=torch.cuda.get_device_name(0),
                timing="device events around each update + render pair, one stream", warmup=args.warmup)
    lines = [json.dumps(head)] + [json.dumps(x) for x in rows]
    print(f"# {N}^3 volume, layout {layout} ({variant}), {W}x{H}x{args.steps}, {head['device']}")
    for x in rows:
        if x["call"] != "edit":
            print(f"  {x['call']:22} umask {x['uniform_mask']:>2} share {x['frame_share']:>9.6f} "
                  f"median {x['median_ms']:.4f} ms (min {x['min_ms']:.4f}, max {x['max_ms']:.4f})")
    print(f"# {'box':>5} {'origin':8} {'umask':>5} {'footprint':>18} {'share':>7} {'update+rect ms':>22} "
          f"{'update+frame ms':>22}  rect faster")
    for x in rows:
        if x["call"] == "edit":
            a, b, q = x["rect_path"], x["frame_path"], x["rect"]
            print(f"  {x['box']:>4}^3 {x['align']:8} {x['uniform_mask']:>5} {q[2]:>5}x{q[3]:<4}@({q[0]:>4},{q[1]:>4}) "
                  f"{x['frame_share']:>7.4f} {a['median_ms']:>8.4f} ({a['min_ms']:.4f}-{a['max_ms']:.4f}) "
                  f"{b['median_ms']:>8.4f} ({b['min_ms']:.4f}-{b['max_ms']:.4f})  {'yes' if x['rect_faster'] else 'NO'}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
