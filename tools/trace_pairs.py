"""The timed window of a plain `rocprofv3 --kernel-trace` run of bench.py (config 5), read
from its kernel_trace.csv: the last K frames' march launches -- one per frame
(march_regions_u) or one per NF frames (march_regions_frames_u<..., NF>: the native loop's pairs,
NF 2, and groups of four, option frame_group 4).  Traces of earlier builds name those kernels
march_regions_pair_u and march_regions_group_u.

    python tools/trace_pairs.py TRACE.csv [--steps 50]

Prints the kernel, launches, frames per launch, mean duration of a full launch, and per frame the
span (first start to last end) and the busy time (union of the launches' intervals).
"""
import argparse
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trace_frames import load, union  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("trace")
ap.add_argument("--steps", type=int, default=50)
a = ap.parse_args()
rows = [r for r in load(a.trace) if "march_regions" in r[2]]


def frames_of(name):
    # march_regions_frames[_u]<layout, wrap, early, zero offsets, [mask,] NF>(vr::FramesArgs<NF>, ...)
    m = re.search(r"march_regions_frames(?:_u)?<[^>]*?(\d+)>", name) or re.search(r"FramesArgs<(\d+)>", name)
    if m:
        return int(m.group(1))
    return 4 if "march_regions_group" in name else 2 if "march_regions_pair" in name else 1


# the launches of the last a.steps frames (a window of groups may end in a pair or a single frame)
win, frames = [], 0
for r in reversed(rows):
    if frames >= a.steps:
        break
    win.append(r)
    frames += frames_of(r[2])
win.reverse()
per = max(frames_of(r[2]) for r in win)
main = [r for r in win if frames_of(r[2]) == per]
span = max(e for _, e, _ in win) - min(s for s, _, _ in win)
print(json.dumps({"kernel": main[-1][2][:60], "launches": len(win), "frames": frames, "frames_per_launch": per,
                  "mean_launch_ms": round(sum(e - s for s, e, _ in main) / len(main) * 1e-6, 5),
                  "span_ms_per_frame": round(span * 1e-6 / frames, 5),
                  "busy_ms_per_frame": round(union([(s, e) for s, e, _ in win]) * 1e-6 / frames, 5)}))
