"""vr_render_group, vr_group_split and the option "frame_group" without a GPU: the entry
points are declared, exported and mirrored with the header's argument lists, the split of
n frames into launches is what the header states, the per-frame argument block keeps a
grouped launch inside the kernarg segment, and the calls refuse bad arguments before they
touch a device."""
import ctypes
import os
import re
import subprocess

import pytest

from volumetricrenderer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volumetricrenderer_amd", "csrc")


def declaration(header, name):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in {header}"
    return [a.strip() for a in m.group(1).split(",")]


def test_render_group_is_declared_exported_and_mirrored():
    args = declaration("vr.h", "vr_render_group")
    assert len(args) == 6 and args[0] == "void* ctx" and args[5] == "void* stream"
    assert args[1].startswith("const vr_target*") and args[2] == "int n"
    assert "vr_object_shader_data" in args[3] and "vr_global_shader_data" in args[4]
    f = getattr(_lib.load(), "vr_render_group")
    assert f.restype is ctypes.c_int and len(f.argtypes) == 6
    assert f.argtypes[1]._type_ is _lib.Target and f.argtypes[2] is ctypes.c_int
    assert f.argtypes[3]._type_ is _lib.ObjectShaderData and f.argtypes[4]._type_ is _lib.GlobalShaderData


def test_group_split():
    """n frames -> launches: 4 -> {4}, 3 -> {2, 1}, 2 -> {2}, 1 -> {1}; anything else 0 launches."""
    assert declaration("vr.h", "vr_group_split") == ["int n", "int launches[3]"]
    split = _lib.load().vr_group_split
    want = {1: [1, 0, 0], 2: [2, 0, 0], 3: [2, 1, 0], 4: [4, 0, 0]}
    for n in range(-1, 7):
        out = (ctypes.c_int * 3)(9, 9, 9)
        k = split(n, out)
        if n in want:
            assert list(out) == want[n] and k == sum(1 for v in want[n] if v) and sum(out) == n
        else:
            assert k == 0 and list(out) == [9, 9, 9]
    assert split(4, None) == 0


def test_frame_group_is_an_option_not_a_shard_entry_point():
    text = open(os.path.join(ROOT, "include", "vr_shard.h")).read()
    assert '"frame_group"' in text
    assert not hasattr(_lib.load_shard(), "vr_shard_set_group")


def test_bad_arguments_are_refused():
    t = (_lib.Target * 4)(*[_lib.Target(width=8, height=8) for _ in range(4)])
    with pytest.raises(_lib.VRError) as e:
        _lib.call("vr_render_group", None, t, 4, None, None, None)
    assert e.value.status == 1   # VR_ERR_INVALID
    with pytest.raises(_lib.VRError):
        _lib.call("vr_set_option", None, b"frame_group", 4)


def test_frame_args_layout(tmp_path):
    """FrameArgs holds exactly the per-frame fields and four of them (a pair's launch: two) travel with
    one MarchArgs and the lists' pointers inside the 4096-B kernarg segment (host compile of vr_internal.h)."""
    hipcc = "/opt/rocm/bin/hipcc"
    src = tmp_path / "t.cpp"
    fields = ["org", "o", "px", "py", "r2", "r3", "cam_mode", "cam", "tap_T", "empty_fill", "out", "step_counter"]
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "vr_internal.h"\nusing namespace vr;\nint main(){'
                   'printf("%zu %zu %zu %d %zu", sizeof(FrameArgs), sizeof(MarchArgs), sizeof(GroupArgs), kGroupFrames,'
                   ' sizeof(FramesArgs<2>));'
                   + "".join('printf(" %%zu %%zu", offsetof(FrameArgs, %s), sizeof(FrameArgs::%s));' % (f, f) for f in fields)
                   + 'MarchArgs a{}; a.org[1] = 3.f; a.tap_T[2][1] = 7.f; a.cam_mode = 1; a.empty_fill = 1; a.max_steps = 5;'
                   'a.out = &a; MarchArgs b{}; b.max_steps = 9; set_frame(&b, frame_part(a));'
                   'printf(" %d", b.org[1] == 3.f && b.tap_T[2][1] == 7.f && b.cam_mode == 1 && b.empty_fill == 1 &&'
                   ' b.out == &a && b.max_steps == 9);return 0;}\n')
    exe = tmp_path / "t"
    subprocess.run([hipcc, "-std=c++17", "-x", "c++", "-I", CSRC, "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                    str(src), "-o", str(exe), "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    frame, march, group, k, pair = got[:5]
    print("FrameArgs", frame, "MarchArgs", march, "FramesArgs<4>", group, "FramesArgs<2>", pair)
    assert k == 4 and group == march + 4 * frame and group + 64 <= 4096
    assert pair == march + 2 * frame
    offs = got[5:-1]
    end = 0
    for i in range(len(fields)):   # in declaration order, no field missing, nothing but alignment padding between
        off, size = offs[2 * i], offs[2 * i + 1]
        assert end <= off < end + 8, fields[i]
        end = off + size
    assert end == frame
    assert got[-1] == 1   # set_frame(frame_part(a)) carries the per-frame fields and nothing else
