"""The timed window of a plain `rocprofv3 --kernel-trace` run of bench.py (config 5), read
from its kernel_trace.csv: the last K frames' march launches -- one per frame
(march_regions_u) or one per pair (march_regions_pair_u, the native loop's paired frames).

    python tools/trace_pairs.py TRACE.csv [--steps 50]

Prints the kernel, launches, frames per launch, mean launch duration, and per frame the
span (first start to last end) and the busy time (union of the launches' intervals).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trace_frames import load, union  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("trace")
ap.add_argument("--steps", type=int, default=50)
a = ap.parse_args()
rows = [r for r in load(a.trace) if "march_regions" in r[2]]
tail = rows[-a.steps:]
paired = sum("march_regions_pair" in r[2] for r in tail) > len(tail) // 2
per = 2 if paired else 1
win = rows[-(a.steps // per):]
span = max(e for _, e, _ in win) - min(s for s, _, _ in win)
print(json.dumps({"kernel": win[-1][2][:60], "launches": len(win), "frames_per_launch": per,
                  "mean_launch_ms": round(sum(e - s for s, e, _ in win) / len(win) * 1e-6, 5),
                  "span_ms_per_frame": round(span * 1e-6 / a.steps, 5),
                  "busy_ms_per_frame": round(union([(s, e) for s, e, _ in win]) * 1e-6 / a.steps, 5)}))
