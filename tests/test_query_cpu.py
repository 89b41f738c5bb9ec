"""vr_query_rect, the checks that need no GPU: the record's layout in
include/vr.h against its ctypes and numpy mirrors, the export and its
prototype, and the argument validation a call reaches without a device (a null
context or pointer: what tests/test_rect_cpu.py and tests/test_rects_cpu.py
reach for the scissored renders).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from volumetricrenderer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VR_ERR_INVALID = 1
FIELDS = ("steps", "hit_step", "value", "optical_depth", "entry", "reserved0", "step", "reserved1", "hit", "reserved2")


def test_record_is_64_bytes_with_the_issue_layout():
    R = _lib.RayRecord
    assert ctypes.sizeof(R) == 64 and _lib.RAY_RECORD_WORDS == 16
    assert [n for n, *_ in R._fields_] == list(FIELDS)
    want = dict(steps=0, hit_step=4, value=8, optical_depth=12, entry=16, reserved0=28, step=32, reserved1=44,
                hit=48, reserved2=60)
    assert {n: getattr(R, n).offset for n in FIELDS} == want


def test_header_record_layout_matches_ctypes(tmp_path):
    """Compile include/vr.h with gcc: sizeof(vr_ray_record) and every field's
    offset equal the ctypes mirror's."""
    src = tmp_path / "record.c"
    offs = ", ".join(f"offsetof(vr_ray_record, {n})" for n in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vr.h"\n'
                   "int main(void){size_t v[] = {sizeof(vr_ray_record), " + offs + "};\n"
                   "for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf(\"%zu \", v[i]);\nreturn 0;}\n")
    exe = tmp_path / "record"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [64] + [getattr(_lib.RayRecord, n).offset for n in FIELDS]


def test_numpy_record_type_matches_ctypes():
    import volumetricrenderer_amd as vr
    dt = vr.RAY_RECORD_DTYPE
    assert dt.itemsize == 64 and dt.names == FIELDS
    assert {n: dt.fields[n][1] for n in FIELDS} == {n: getattr(_lib.RayRecord, n).offset for n in FIELDS}
    rec = _lib.RayRecord(steps=7, hit_step=-1, value=0.25, optical_depth=1.5)
    rec.entry[:] = [0.1, 0.2, 0.3]
    rec.step[:] = [-1.0, 2.0, 0.5]
    words = np.frombuffer(bytes(rec), np.int32).reshape(1, 1, 16).copy()
    r = vr.ray_records(words)
    assert r.shape == (1, 1)
    assert r["steps"][0, 0] == 7 and r["hit_step"][0, 0] == -1 and r["value"][0, 0] == np.float32(0.25)
    assert r["optical_depth"][0, 0] == np.float32(1.5)
    assert r["entry"][0, 0].tolist() == [np.float32(0.1), np.float32(0.2), np.float32(0.3)]
    assert r["step"][0, 0].tolist() == [-1.0, 2.0, 0.5] and r["hit"][0, 0].tolist() == [0.0, 0.0, 0.0]
    for bad in (np.zeros((2, 2, 15), np.int32), np.zeros((2, 2, 16), np.float32)):
        with pytest.raises(ValueError):
            vr.ray_records(bad)


def test_header_declares_the_prototype():
    src = open(os.path.join(ROOT, "include", "vr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"vr_status\s+vr_query_rect\s*\(\s*void\*\s*ctx,\s*int\s+width,\s*int\s+height,\s*"
                     r"const vr_rect\*\s*rect,\s*float\s+threshold,\s*void\*\s*d_records,\s*"
                     r"size_t\s+row_pitch_records,\s*void\*\s*stream\s*\)\s*;", src)
    hpp = open(os.path.join(ROOT, "include", "vr_renderer.hpp")).read()
    assert "QueryRect" in hpp and "vr_query_rect" in hpp


def test_export_and_null_arguments():
    lib = _lib.load()
    assert hasattr(lib, "vr_query_rect") and "vr_query_rect" in _lib.exported_symbols()
    assert lib.vr_query_rect.restype is ctypes.c_int and len(lib.vr_query_rect.argtypes) == 8
    assert lib.vr_abi_version() == 2   # additions only
    rect = _lib.Rect(0, 0, 1, 1)
    rec = _lib.RayRecord(steps=-7, hit_step=-7)
    before = bytes(rec)
    # a null context, with and without the other pointers: refused before anything is read or written
    for r, d in ((ctypes.byref(rect), ctypes.byref(rec)), (None, ctypes.byref(rec)), (ctypes.byref(rect), None),
                 (None, None)):
        assert lib.vr_query_rect(None, 64, 48, r, 0.0, d, 0, None) == VR_ERR_INVALID
        assert b"vr_query_rect" in lib.vr_last_error()
    assert bytes(rec) == before
    with pytest.raises(_lib.VRError) as e:
        _lib.call("vr_query_rect", None, 64, 48, ctypes.byref(rect), 0.5, ctypes.byref(rec), 0, None)
    assert e.value.status == VR_ERR_INVALID and "vr_query_rect" in str(e.value)
