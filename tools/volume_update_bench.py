#!/usr/bin/env python3
"""Cost of a partial volume update against the full install.

A 512^3 recipe volume on the auto layout; vr_update_volume_device for boxes of
16^3, 64^3, 128^3, 256^3 (1/8 of the texels) and the whole volume, at an
aligned and an odd origin, and vr_set_volume_device of the whole volume in the
same process -- the only way to change a texel without the update call, hence
the baseline.  Each call is timed with device events on one stream, after
warm-up calls of the same shape; the table gives the median, the minimum and
the maximum.  Two passes: with the recipe's uniform G still held (every update
re-arms the min / max read-back) and after one texel has broken it (the
steady state of a time-varying volume: launches only).

The one condition checked (exit status 1): every box with at most 1/8 of the
texels updates in less time than the full install of the same run.

    python tools/volume_update_bench.py [--size 512] [--reps 25] [--out FILE]
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


def timed(fn, stream, warmup, reps):
    """Milliseconds of each of `reps` calls of fn() on `stream` (device events)."""
    for _ in range(warmup):
        fn()
    stream.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("volume_update_bench: no GPU", file=sys.stderr)
        return 2
    if args.reps < 20:
        ap.error("--reps: the median of at least 20")
    N = args.size
    rows = []
    with vr.Renderer(0) as r:
        r.generate_volume(vr.scaled_recipe(N))
        layout = r.get_option("layout")
        osd, gsd = vr.reference_shader_data(16 / 9)
        r.set_shader_data(osd, gsd)
        variant = r.kernel_variant
        vol = torch.from_numpy(r.get_volume()).cuda()
        s = torch.cuda.Stream()
        sh = ctypes.c_void_p(s.cuda_stream)
        ctx = r._ctx
        edges = [e for e in (16, 64, 128, 256) if e < N] + [N]
        odd = (N // 4 + 1, N // 4 + 3, N // 4 + 5)
        cases = []
        for e in edges:
            for tag, o in (("aligned", (N // 4,) * 3), ("odd", odd)):
                if e == N:
                    if tag == "odd":
                        continue
                    o = (0, 0, 0)
                if max(o) + e > N:
                    continue
                box = vol[o[2]:o[2] + e, o[1]:o[1] + e, o[0]:o[0] + e].contiguous()
                cases.append((e, tag, o, box))
        torch.cuda.synchronize()

        def install():
            _lib.call("vr_set_volume_device", ctx, ctypes.c_void_p(vol.data_ptr()), N, N, N, sh)

        for held in (True, False):
            r.set_volume_device(vol, stream=s)
            if not held:   # one texel breaks the uniform channel(s); resolve it before timing
                t = vol[:1, :1, :1].clone()
                t[..., :] = 255 - t
                r.update_volume(t, (0, 0, 0), stream=s)
                s.synchronize()
            mask = r.get_option("uniform_mask")
            for e, tag, o, box in cases:
                ms = timed(lambda: _lib.call("vr_update_volume_device", ctx, ctypes.c_void_p(box.data_ptr()), *o, e, e,
                                             e, sh), s, args.warmup, args.reps)
                rows.append(dict(call="update", box=e, origin=list(o), align=tag, uniform_mask=mask,
                                 texel_share=e ** 3 / N ** 3, median_ms=statistics.median(ms), min_ms=min(ms),
                                 max_ms=max(ms), reps=len(ms)))
                if not held:
                    assert r.get_option("uniform_mask") == 0
        ms = timed(install, s, args.warmup, args.reps)
        s.synchronize()
        base = dict(call="install", box=N, origin=[0, 0, 0], align="aligned", uniform_mask=-1, texel_share=1.0,
                    median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms))
        rows.append(base)
    head = dict(tool="volume_update_bench", size=N, layout=layout, variant=variant, device=torch.cuda.get_device_name(0),
                timing="device events around each call, one stream", warmup=args.warmup)
    lines = [json.dumps(head)] + [json.dumps(x) for x in rows]
    print(f"# {N}^3 volume, layout {layout} ({variant}), {head['device']}")
    print(f"# {'call':8} {'box':>5} {'origin':8} {'umask':>5} {'share':>8} {'median ms':>10} {'min':>8} {'max':>8}")
    for x in rows:
        print(f"  {x['call']:8} {x['box']:>4}^3 {x['align']:8} {x['uniform_mask']:>5} {x['texel_share']:>8.5f} "
              f"{x['median_ms']:>10.4f} {x['min_ms']:>8.4f} {x['max_ms']:>8.4f}")
    slow = [x for x in rows if x["call"] == "update" and x["texel_share"] <= 0.125
            and not x["median_ms"] < base["median_ms"]]
    verdict = dict(condition="update of <= 1/8 of the texels faster than the full install", holds=not slow,
                   install_median_ms=base["median_ms"])
    lines.append(json.dumps(verdict))
    print(json.dumps(verdict))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
