"""vr_render_pair and the option "frame_pairing" without a GPU: the entry point is
declared, exported and mirrored with the header's argument list, the target
structure the pair call takes twice has the header's layout, and the calls
refuse bad arguments before they touch a device."""
import ctypes
import os
import re
import subprocess

import pytest

from volumetricrenderer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declaration(header, name):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in {header}"
    return [a.strip() for a in m.group(1).split(",")]


def test_render_pair_is_declared_exported_and_mirrored():
    args = declaration("vr.h", "vr_render_pair")
    assert len(args) == 6 and args[0] == "void* ctx" and args[5] == "void* stream"
    assert args[1].startswith("const vr_target*") and args[2].startswith("const vr_target*")
    assert "vr_object_shader_data" in args[3] and "vr_global_shader_data" in args[4]
    res, sig = _lib._SIGS["vr_render_pair"] if hasattr(_lib, "_SIGS") else (None, None)
    f = getattr(_lib.load(), "vr_render_pair")
    assert f.restype is ctypes.c_int and len(f.argtypes) == 6
    assert f.argtypes[1] is f.argtypes[2] and f.argtypes[1]._type_ is _lib.Target
    assert f.argtypes[3]._type_ is _lib.ObjectShaderData and f.argtypes[4]._type_ is _lib.GlobalShaderData
    if sig is not None:
        assert res is ctypes.c_int and list(sig) == list(f.argtypes)


def test_frame_pairing_is_an_option_not_a_shard_entry_point():
    """The loop's switch is the context's option "frame_pairing": vr_shard.h documents it and
    gains no function."""
    text = open(os.path.join(ROOT, "include", "vr_shard.h")).read()
    assert '"frame_pairing"' in text
    assert not hasattr(_lib.load_shard(), "vr_shard_set_pairing")


def test_pair_target_layout_matches_header(tmp_path):
    """vr_target, every field: the pair call reads two of them."""
    fields = [n for n, _ in _lib.Target._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vr.h"\nint main(void){printf("%zu", sizeof(vr_target));'
                   + "".join('printf(" %%zu", offsetof(vr_target, %s));' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.Target)] + [getattr(_lib.Target, f).offset for f in fields]


def test_null_arguments_are_refused():
    t = _lib.Target(width=8, height=8)
    with pytest.raises(_lib.VRError) as e:
        _lib.call("vr_render_pair", None, ctypes.byref(t), ctypes.byref(t), None, None, None)
    assert e.value.status == 1   # VR_ERR_INVALID
    with pytest.raises(_lib.VRError):
        _lib.call("vr_set_option", None, b"frame_pairing", 1)
