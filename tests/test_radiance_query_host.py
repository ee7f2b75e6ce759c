"""CPU: the radiance-query records (include/urt_types.h urt_PathRay / urt_PathPixel) have one layout in the header, in _lib's ctypes
structures, in the numpy records of unity_api and in a C compiler's offsetof; Context.radiance_query / radiance_query_pixels validate
their arguments before they call the library; and without a GPU nothing computes: a context — the only way to the entry points — is
refused with URT_ERR_NO_DEVICE, and the entry points themselves refuse a NULL context."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import unityraytracer_amd as urt
from unityraytracer_amd import _lib, unity_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

PATHRAY_FIELDS = {"origin": 0, "seed": 12, "direction": 16, "reserved0": 28, "px": 32, "py": 36, "reserved1": 40}
PATHPIXEL_FIELDS = {"x": 0, "y": 4}


def test_struct_sizes_match_the_strides():
    text = open(os.path.join(ROOT, "include", "urt_types.h")).read()
    assert "#define URT_STRIDE_PATHRAY 48" in text and "#define URT_STRIDE_PATHPIXEL 8" in text
    assert C.sizeof(_lib.PathRay) == 48 == _lib.URT_STRIDE_PATHRAY == unity_api.PATHRAY_DT.itemsize
    assert C.sizeof(_lib.PathPixel) == 8 == _lib.URT_STRIDE_PATHPIXEL == unity_api.PATHPIXEL_DT.itemsize
    for cls, dt, fields in ((_lib.PathRay, unity_api.PATHRAY_DT, PATHRAY_FIELDS), (_lib.PathPixel, unity_api.PATHPIXEL_DT, PATHPIXEL_FIELDS)):
        assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == fields
        assert {n: dt.fields[n][1] for n in dt.names} == fields


def test_a_c_compiler_sees_the_same_layout(tmp_path):
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "urt.h"', 'int main(void) {']
    for struct, fields in (("urt_PathRay", PATHRAY_FIELDS), ("urt_PathPixel", PATHPIXEL_FIELDS)):
        lines.append(f'  printf("{struct} size %zu\\n", sizeof({struct}));')
        for f in fields:
            lines.append(f'  printf("{struct} {f} %zu\\n", offsetof({struct}, {f}));')
    lines += ['  printf("flags %d %d\\n", URT_RADIANCE_RAYS, URT_RADIANCE_PIXELS);', '  return 0;', '}']
    (tmp_path / "probe.c").write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")],
                   check=True)
    got = {}
    for line in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.splitlines():
        a, b, c = line.split(" ", 2)
        got[(a, b)] = c
    assert got[("urt_PathRay", "size")] == "48" and got[("urt_PathPixel", "size")] == "8"
    for struct, fields in (("urt_PathRay", PATHRAY_FIELDS), ("urt_PathPixel", PATHPIXEL_FIELDS)):
        for f, off in fields.items():
            assert got[(struct, f)] == str(off), (struct, f)
    assert got[("flags", "0")] == "1"
    assert (_lib.URT_RADIANCE_RAYS, _lib.URT_RADIANCE_PIXELS) == (0, 1)


def test_header_binding_and_csharp_declare_the_entry_points():
    text = open(os.path.join(ROOT, "include", "urt.h")).read()
    assert re.search(r"URT_RADIANCE_RAYS\s*=\s*0", text) and re.search(r"URT_RADIANCE_PIXELS\s*=\s*1", text)
    assert "urt_radiance_query(" in text and "urt_radiance_query_device(" in text
    assert {"urt_radiance_query", "urt_radiance_query_device"} <= set(_lib.ABI_SYMBOLS)
    cs = open(os.path.join(ROOT, "integration", "UrtNative.cs")).read()
    assert "urt_radiance_query(" in cs and "urt_radiance_query_device(" in cs and "struct PathRay" in cs and "struct PathPixel" in cs
    assert "class UrtRadiance" in open(os.path.join(ROOT, "integration", "UrtUnityShim.cs")).read()
    assert "URT_API int urt_abi_version" in text and _lib.load().urt_abi_version() == 4     # nothing that existed changed


class _StubLib:
    """Records the calls the wrappers make instead of reaching a GPU."""

    def __init__(self):
        self.calls = []

    def urt_radiance_query(self, h, inp, n, samples, bounces, out, flags):
        stride = 8 if flags == 1 else 48
        self.calls.append((n, samples, bounces, flags, bytes(C.string_at(inp, stride * n)) if n else b""))
        return 0

    def urt_radiance_query_device(self, *a):
        self.calls.append(a)
        return 0


def stub_context():
    ctx = object.__new__(unity_api.Context)
    ctx.lib = _StubLib()
    ctx._h = C.c_void_p(1)
    ctx.device = 0
    return ctx


def good(n=4):
    return dict(origins=np.zeros((n, 3), F), directions=np.ones((n, 3), F), pixels=np.zeros((n, 2), F), seeds=0.25, samples=2, bounces=3)


@pytest.mark.parametrize("change, exc", [
    (dict(origins=np.zeros((4, 3), np.float64)), TypeError),          # float64: no silent rounding of the caller's rays
    (dict(directions=np.zeros((4, 3), np.int32)), TypeError),
    (dict(origins=np.zeros((4, 4), F), directions=np.zeros((4, 4), F)), ValueError),
    (dict(origins=np.zeros(12, F)), ValueError),
    (dict(directions=np.zeros((5, 3), F)), ValueError),
    (dict(origins=[[0, 0, 0]] * 4), TypeError),
    (dict(pixels=np.zeros((4, 2), np.int32)), TypeError),
    (dict(pixels=np.zeros((4, 3), F)), ValueError),
    (dict(pixels=np.zeros((3, 2), F)), ValueError),
    (dict(pixels=[(0, 0)] * 4), TypeError),
    (dict(seeds=np.zeros(3, F)), ValueError),
    (dict(seeds=np.zeros(4, np.float64)), TypeError),
    (dict(seeds="one"), TypeError),
    (dict(samples=0), ValueError), (dict(samples=4097), ValueError), (dict(samples=1.0), TypeError), (dict(samples=True), TypeError),
    (dict(bounces=-1), ValueError), (dict(bounces=65), ValueError), (dict(bounces=2.0), TypeError),
])
def test_radiance_query_validates_before_calling_the_library(change, exc):
    ctx = stub_context()
    args = good()
    args.update(change)
    with pytest.raises(exc):
        ctx.radiance_query(**args)
    assert ctx.lib.calls == []


@pytest.mark.parametrize("xy, samples, bounces, exc", [
    (np.zeros((4, 2), np.int64), 1, 1, TypeError),
    (np.zeros((4, 2), F), 1, 1, TypeError),
    (np.zeros((4, 3), np.int32), 1, 1, ValueError),
    (np.zeros(8, np.int32), 1, 1, ValueError),
    ([(0, 0)], 1, 1, TypeError),
    (np.zeros((4, 2), np.int32), 0, 1, ValueError),
    (np.zeros((4, 2), np.int32), 4097, 1, ValueError),
    (np.zeros((4, 2), np.int32), 1, 65, ValueError),
    (np.zeros((4, 2), np.int32), 1, -1, ValueError),
    (np.zeros((4, 2), np.int32), "1", 1, TypeError),
])
def test_radiance_query_pixels_validates_before_calling_the_library(xy, samples, bounces, exc):
    ctx = stub_context()
    with pytest.raises(exc):
        ctx.radiance_query_pixels(xy, samples, bounces)
    assert ctx.lib.calls == []


def test_wrappers_pack_the_records():
    ctx = stub_context()
    o = np.array([[1, 2, 3], [4, 5, 6]], F)
    d = np.array([[0, -1, 0], [1, 0, 0]], F)
    p = np.array([[7, 8], [9.5, 10]], F)
    out = ctx.radiance_query(o, d, p, np.array([0.25, 0.75], F), 16, 8)
    assert out.dtype == F and out.shape == (2, 4)
    n, samples, bounces, flags, raw = ctx.lib.calls[0]
    assert (n, samples, bounces, flags) == (2, 16, 8, 0)
    rec = np.frombuffer(raw, dtype=F).reshape(2, 12)
    assert np.array_equal(rec[:, 0:3], o) and np.array_equal(rec[:, 4:7], d) and np.array_equal(rec[:, 8:10], p)
    assert rec[:, 3].tolist() == [0.25, 0.75] and not rec[:, [7, 10, 11]].view(np.int32).any()
    ctx.radiance_query(o, d, p, 0.5, 1, 0)                                # a scalar seed goes to every ray; bounces 0 and samples 1 are in range
    assert np.frombuffer(ctx.lib.calls[1][4], dtype=F).reshape(2, 12)[:, 3].tolist() == [0.5, 0.5]
    xy = np.array([[3, 4], [0, 0], [39, 23]], np.int32)
    out = ctx.radiance_query_pixels(xy[:, ::-1][:, ::-1], 4096, 64)       # a non-contiguous view is packed, not refused
    assert out.shape == (3, 4) and ctx.lib.calls[2][:4] == (3, 4096, 64, 1)
    assert np.array_equal(np.frombuffer(ctx.lib.calls[2][4], dtype=np.int32).reshape(3, 2), xy)
    assert ctx.radiance_query_pixels(np.zeros((0, 2), np.int32), 1, 1).shape == (0, 4)


def test_no_device_no_result(built_library):
    """No CPU fallback: on a machine without a GPU the context every query needs is refused with URT_ERR_NO_DEVICE; the entry points
    refuse a NULL context whatever the machine, before they look at anything else."""
    import torch
    lib = _lib.load()
    rays, out = (C.c_float * 12)(), (C.c_float * 4)(*([7.0] * 4))
    for fn in (lib.urt_radiance_query, lib.urt_radiance_query_device):
        for flags in (0, 1):
            assert fn(None, rays, 1, 1, 1, out, flags) == 1               # URT_ERR_INVALID_ARGUMENT
    assert list(out) == [7.0] * 4
    if not torch.cuda.is_available():
        with pytest.raises(urt.UrtError) as e:
            urt.Context(0)
        assert e.value.code == 3 and "no CPU fallback" in str(e.value)   # URT_ERR_NO_DEVICE
