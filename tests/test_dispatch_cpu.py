"""The march launchers' compile-time dispatcher (csrc/vr_dispatch.h), the checks
that need no GPU: tools/dispatch_check.cpp -- the dispatcher, the layout lists
and the _u / LDS rules of vr_internal.h behind a main of their own -- built by
tools/Makefile for the default and the EXPERIMENTS=1 lists and run; and the
launch macros the dispatcher replaced stay gone from csrc.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volumetricrenderer_amd", "csrc")


@pytest.mark.parametrize("experiments", [0, 1])
def test_dispatch_check_builds_and_passes(tmp_path, experiments):
    exe = tmp_path / "dispatch_check"
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), f"DISPATCH_CHECK={exe}", f"EXPERIMENTS={experiments}",
                    str(exe)], check=True, capture_output=True, text=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert f"dispatch_check: ok (VR_EXPERIMENTS={experiments})" in p.stdout


def test_no_launch_macros_in_csrc():
    """No #define VR_R* / VR_U* / VR_P* in csrc takes arguments and launches a kernel, and the launch
    macros the dispatcher replaced stay gone."""
    gone = {"VR_RW", "VR_UM", "VR_UMS", "VR_UMF", "VR_PD", "VR_PS", "VR_PS3", "VR_PT", "VR_PR"}
    found = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".h", ".hip", ".cpp")):
            continue
        text = open(os.path.join(CSRC, name)).read()
        for m in re.finditer(r"#\s*define\s+(VR_[RUP]\w*)(\()?([^\n]*(?:\\\n[^\n]*)*)", text):
            macro, params, body = m.group(1), m.group(2), m.group(3)
            if macro in gone or (params and "hipLaunchKernelGGL" in body):
                found.append((name, macro))
    assert not found, found


def test_no_retired_build_knobs_in_csrc():
    """The build knobs whose measured winner became the plain code are named
    nowhere in csrc, comments included: the record of what they tried is DESIGN.md's."""
    retired = ["VR_PIPE", "VR_LANEMAP", "VR_PROC_WAVES", "VR_PROC_ATTR", "VR_DEFER_UNROLL", "VR_DEFER_ATTR",
               "VR_FBM_UNROLL", "VR_FBM_UNROLL_BY", "VR_FBM_PREFETCH", "VR_FBM_FENCE", "VR_PROC_PHASES",
               "VR_PHASE_FENCE", "VR_UM_ATTR", "VR_UM_WAVES", "VR_SHADOW_PHASED", "VR_SHADOW_WAVES",
               "VR_SHADOW_ATTR", "VR_CUBE_BATCH"]
    pattern = re.compile(r"\b(" + "|".join(retired) + r")\b")
    found = []
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if not os.path.isfile(path) or name.endswith((".o", ".so")):
            continue
        for m in pattern.finditer(open(path, errors="replace").read()):
            found.append((name, m.group(1)))
    assert not found, found
