"""Partial volume updates (vr_update_volume / vr_update_volume_device), the
checks that need no GPU: the header, the ctypes table and the library all
carry the two entry points with the same signatures, and the argument checks
that come before any device work answer without one."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vr_update_volume", "vr_update_volume_device")


def header_source():
    src = open(os.path.join(ROOT, "include", "vr.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_ctypes_and_library_carry_both_symbols():
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    declared = set(re.findall(r"\b(vr_[a-z_0-9]+)\s*\(", header_source()))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    # the ctypes signatures: ctx, data, six ints (origin, extent) [, stream], returning a vr_status
    ints = [ctypes.c_int] * 6
    assert _lib._SIGS["vr_update_volume"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p] + ints)
    assert _lib._SIGS["vr_update_volume_device"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p] + ints
                                                     + [ctypes.c_void_p])
    # ... and the header's parameter lists say the same
    src = header_source()
    for name, nargs in (("vr_update_volume", 8), ("vr_update_volume_device", 9)):
        m = re.search(r"vr_status\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == nargs
        assert params[0].startswith("void*") and all(p.startswith("int ") for p in params[2:8])
        assert len(_lib._SIGS[name][1]) == nargs


def test_header_declarations_compile_as_c(tmp_path):
    """include/vr.h with the new declarations is still plain C99, and a call
    through them links against libvr.so and is refused cleanly (in the style
    of test_header_layouts_match_ctypes)."""
    src = tmp_path / "upd.c"
    src.write_text(
        '#include <stdio.h>\n#include "vr.h"\n'
        "int main(void){\n"
        "  unsigned char t[4] = {0, 0, 0, 0};\n"
        "  int a = vr_update_volume(NULL, t, 0, 0, 0, 1, 1, 1);\n"
        "  int b = vr_update_volume_device(NULL, t, 0, 0, 0, 1, 1, 1, NULL);\n"
        '  printf("%d %d %d\\n", a, b, vr_abi_version());\n'
        "  return 0;}\n")
    exe = tmp_path / "upd"
    libdir = os.path.join(ROOT, "volumetricrenderer_amd")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lvr", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["1", "1", "2"]


def test_null_arguments_are_invalid_with_a_message():
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    texel = (ctypes.c_uint8 * 4)()
    for name, extra in (("vr_update_volume", ()), ("vr_update_volume_device", (None,))):
        f = getattr(lib, name)
        assert f(None, texel, 0, 0, 0, 1, 1, 1, *extra) == 1   # VR_ERR_INVALID
        msg = lib.vr_last_error().decode()
        assert name in msg and "null" in msg
    try:
        _lib.call("vr_update_volume", None, None, 0, 0, 0, 1, 1, 1)
    except _lib.VRError as e:
        assert e.status == 1 and "vr_update_volume" in str(e)
    else:
        raise AssertionError("vr_update_volume(NULL, ...) was accepted")


def test_abi_version_is_still_2():
    from volumetricrenderer_amd import _lib
    assert _lib.load().vr_abi_version() == 2
    assert re.search(r"#define\s+VR_ABI_VERSION\s+2\b", open(os.path.join(ROOT, "include", "vr.h")).read())
