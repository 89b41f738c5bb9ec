#!/usr/bin/env python3
"""What a full plane of ray records costs: whole-frame vr_query_rect against
whole-frame vr_render_rect and vr_render.

A 512^3 recipe volume on the auto layout at 1920 x 1080 x 128 steps with the
reference camera, one process, one stream, device events around each call,
warm-up calls of the same shape first; per call the median, minimum and
maximum in ms.  Two passes: with the recipe's uniform G still held, and after
one texel has broken it.  Also checks that the records' `value` is the R32F
frame bit for bit.  No ratio is required; exits 0 when it ran.

    python tools/query_rect_bench.py [--size 512] [--reps 25] [--out FILE]
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
    return [statistics.median(ms), min(ms), max(ms)]


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
        print("query_rect_bench: no GPU", file=sys.stderr)
        return 2
    N, W, H = args.size, args.width, args.height
    out = dict(tool="query_rect_bench", size=N, width=W, height=H, steps=args.steps, reps=args.reps,
               warmup=args.warmup, columns="median_ms, min_ms, max_ms")
    with vr.Renderer(0) as r:
        r.generate_volume(vr.scaled_recipe(N))
        osd, gsd = vr.reference_shader_data(W / H)
        r.set_shader_data(osd, gsd)
        r.set_march(vr.march_defaults(max_steps=args.steps))
        s = torch.cuda.Stream()
        sh = ctypes.c_void_p(s.cuda_stream)
        ctx = r._ctx
        rect = _lib.Rect(0, 0, W, H)
        rec = torch.empty((H, W, _lib.RAY_RECORD_WORDS), dtype=torch.int32, device="cuda")
        for broken in (False, True):
            if broken:   # one texel breaks the uniform channel(s); resolve it before timing
                t = torch.from_numpy(r.get_volume()[:1, :1, :1].copy()).cuda()
                t[...] = 255 - t
                r.update_volume(t, (0, 0, 0), stream=s)
                s.synchronize()
            for fmt, name in ((vr.FMT_R32F, "r32f"), (vr.FMT_RGBA8_UNORM, "rgba8")):
                frame = r.alloc_target(W, H, fmt)
                target = _lib.Target(width=W, height=H, format=fmt, band_rows=0, band_stride=1, band_first=0,
                                     pixels=frame.data_ptr(), row_pitch=frame.stride(0) * frame.element_size(),
                                     step_counter=None)
                r.render(W, H, fmt, out=frame)
                torch.cuda.synchronize()
                key = f"umask{r.get_option('uniform_mask')}_{name}"
                out[key + "_render_rect"] = summary(timed(
                    lambda: _lib.call("vr_render_rect", ctx, ctypes.byref(target), ctypes.byref(rect), sh), s,
                    args.warmup, args.reps))
                out[key + "_render"] = summary(timed(lambda: _lib.call("vr_render", ctx, ctypes.byref(target), sh), s,
                                                     args.warmup, args.reps))
            for thr in (0.0, 0.5):
                out[f"umask{r.get_option('uniform_mask')}_query_thr{thr}"] = summary(timed(
                    lambda: _lib.call("vr_query_rect", ctx, W, H, ctypes.byref(rect), ctypes.c_float(thr),
                                      ctypes.c_void_p(rec.data_ptr()), 0, sh), s, args.warmup, args.reps))
        out["variant"] = r.kernel_variant
        out["layout"] = r.get_option("layout")
        out["device"] = torch.cuda.get_device_name(0)
        frame = r.render(W, H, vr.FMT_R32F)
        torch.cuda.synchronize()
        out["value_equal"] = bool(torch.equal(rec[..., 2], frame.view(torch.int32)))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
