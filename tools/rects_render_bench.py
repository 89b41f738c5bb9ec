#!/usr/bin/env python3
"""The K-edit loop: K volume updates per frame, then the frame brought up to
date in one of three ways.

The setup is that of tools/rect_render_bench.py: a 512^3 recipe volume on the
auto layout at 1920 x 1080 x 128 steps with the reference camera, RGBA8.  For
K in {1, 4, 16, 64}, K disjoint 16^3 texel boxes at seeded random origins
(multiples of 16; the seed is in the record).  Per K, in one process and on one
stream, device events around the whole sequence:

* (a) K x [vr_update_volume_device + vr_render_rect(footprint)];
* (b) K x vr_update_volume_device, then one vr_render_rects(footprints);
* (c) K x vr_update_volume_device, then one vr_render of the frame.

Each sequence is timed after warm-up runs of the same shape; the record keeps
the median, the minimum and the maximum.  Two passes, as rect_render_bench:
with the recipe's uniform G still held, and after one texel has broken it.
Per K the tool also prints the union of the footprints as a share of the
frame, their overlap (the sum of the rectangle areas over the union's area)
and which sequence was the fastest.  No figure is required: it exits 0 when it ran.

The measurement runs in a child process under a time limit; a child that
fails or runs out of time ends the tool with its status, and nothing more is
started.

    python tools/rects_render_bench.py [--size 512] [--reps 25] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "rects_render", "rects_render_bench.jsonl")
KS = (1, 4, 16, 64)
BOX = 16


def summary(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms))


def disjoint_origins(rng, n, k):
    """k distinct BOX-aligned origins of an n^3 volume: the boxes are disjoint."""
    cells = n // BOX
    picks = rng.choice(cells ** 3, size=k, replace=False)
    return [(int(p % cells) * BOX, int(p // cells % cells) * BOX, int(p // (cells * cells)) * BOX) for p in picks]


def worker(args) -> int:
    import numpy as np
    import torch

    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd import _lib
    from volume_update_bench import timed

    if not torch.cuda.is_available():
        print("rects_render_bench: no GPU", file=sys.stderr)
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
        rng = np.random.default_rng(args.seed)
        cases = []
        for k in KS:
            origins = disjoint_origins(rng, N, k)
            boxes = [vol[o[2]:o[2] + BOX, o[1]:o[1] + BOX, o[0]:o[0] + BOX].contiguous() for o in origins]
            fps = (_lib.Rect * k)()
            for i, o in enumerate(origins):
                _lib.call("vr_update_footprint", ctx, W, H, *o, BOX, BOX, BOX, ctypes.byref(fps[i]))
            mask = np.zeros((H, W), bool)
            area = 0
            for q in fps:
                mask[q.y:q.y + q.height, q.x:q.x + q.width] = True
                area += q.width * q.height
            union = int(mask.sum())
            cases.append(dict(k=k, origins=origins, boxes=boxes, fps=fps, union_px=union, rect_px=area))
        torch.cuda.synchronize()

        def updates(c):
            for o, box in zip(c["origins"], c["boxes"]):
                _lib.call("vr_update_volume_device", ctx, ctypes.c_void_p(box.data_ptr()), *o, BOX, BOX, BOX, sh)

        def seq_a(c):
            for i, (o, box) in enumerate(zip(c["origins"], c["boxes"])):
                _lib.call("vr_update_volume_device", ctx, ctypes.c_void_p(box.data_ptr()), *o, BOX, BOX, BOX, sh)
                _lib.call("vr_render_rect", ctx, ctypes.byref(target), ctypes.byref(c["fps"][i]), sh)

        def seq_b(c):
            updates(c)
            _lib.call("vr_render_rects", ctx, ctypes.byref(target), c["fps"], c["k"], sh)

        def seq_c(c):
            updates(c)
            _lib.call("vr_render", ctx, ctypes.byref(target), sh)

        for held in (True, False):
            r.set_volume_device(vol, stream=s)
            if not held:   # one texel breaks the uniform channel(s); resolve it before timing
                t = vol[:1, :1, :1].clone()
                t[..., :] = 255 - t
                r.update_volume(t, (0, 0, 0), stream=s)
                s.synchronize()
            umask = r.get_option("uniform_mask")
            rows.append(dict(call="render", uniform_mask=umask,
                             **summary(timed(lambda: _lib.call("vr_render", ctx, ctypes.byref(target), sh), s,
                                             args.warmup, args.reps))))
            for c in cases:
                t3 = {name: summary(timed(lambda f=f: f(c), s, args.warmup, args.reps))
                      for name, f in (("a_k_render_rect", seq_a), ("b_one_render_rects", seq_b),
                                      ("c_one_render", seq_c))}
                fastest = min(t3, key=lambda n: t3[n]["median_ms"])
                rows.append(dict(call="k_edits", k=c["k"], box=BOX, uniform_mask=umask, origins=c["origins"],
                                 rects=[[q.x, q.y, q.width, q.height] for q in c["fps"]],
                                 union_share=c["union_px"] / (W * H),
                                 overlap=c["rect_px"] / c["union_px"] if c["union_px"] else None,
                                 fastest=fastest, **t3))
        s.synchronize()
    head = dict(tool="rects_render_bench", size=N, width=W, height=H, steps=args.steps, format=fmt, layout=layout,
                variant=variant, seed=args.seed, device=torch.cuda.get_device_name(0),
                timing="device events around each whole sequence, one stream", warmup=args.warmup)
    print(f"# {N}^3 volume, layout {layout} ({variant}), {W}x{H}x{args.steps}, seed {args.seed}, {head['device']}")
    print(f"# {'K':>3} {'umask':>5} {'union':>8} {'overlap':>7} {'(a) K x render_rect ms':>28} "
          f"{'(b) one render_rects ms':>28} {'(c) one render ms':>28}  fastest")
    for x in rows:
        if x["call"] == "render":
            print(f"  vr_render alone, umask {x['uniform_mask']}: median {x['median_ms']:.4f} ms "
                  f"(min {x['min_ms']:.4f}, max {x['max_ms']:.4f})")
            continue
        cols = " ".join(f"{x[n]['median_ms']:>10.4f} ({x[n]['min_ms']:.4f}-{x[n]['max_ms']:.4f})"
                        for n in ("a_k_render_rect", "b_one_render_rects", "c_one_render"))
        print(f"  {x['k']:>3} {x['uniform_mask']:>5} {x['union_share']:>8.5f} {x['overlap']:>7.3f} {cols}  "
              f"{x['fastest'][0]}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join([json.dumps(head)] + [json.dumps(x) for x in rows]) + "\n")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20240622)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds the measurement may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # the GPU step: a fresh child under its own time limit; its failure is the tool's
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"] + [a for a in sys.argv[1:] if a != "--worker"]
    try:
        return subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        print(f"rects_render_bench: the measurement ran past {args.limit:.0f} s and was ended", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
