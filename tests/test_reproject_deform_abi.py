"""CPU: per-vertex motion for the temporal reprojection (include/urt.h urt_reproject_deformed, urt_buffer_copy) — the header compiles as
C99 and urt_ReprojectDeform has one layout in gcc and ctypes, the symbols are exported and declared in the C# binding, a NULL context is
rejected without a device, and the Python wrappers (Context.reproject(deform=...), reproject_arrays, ComputeBuffer.CopyFrom,
RayTraceMaster.DeformMeshes / SkinMeshes keep_history) validate before they call the library."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from unityraytracer_amd import RayTraceMaster, _lib, unity_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
IMAGE_FIELDS = ("prev_color", "prev_count", "prev_hit", "prev_normal", "prev_id", "hit", "normal", "id", "color", "count", "motion")
DEFORM_FIELDS = ("prev_vertices", "indices", "prev_mesh_objects", "deformed", "normal_threshold", "flags")


# ---- 1. the ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(tmp_path):
    inc = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
    src = tmp_path / "layout.c"
    offs = ", ".join(f"offsetof(urt_ReprojectDeform, {f})" for f in DEFORM_FIELDS)
    src.write_text('#include "urt.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int (*fn)(urt_context*, const urt_ReprojectImages*, const urt_ReprojectParams*, const urt_ReprojectMotion*, '
                   'const urt_ReprojectDeform*) = urt_reproject_deformed;\n'
                   'int (*fc)(urt_context*, urt_handle, int, urt_handle, int, int) = urt_buffer_copy;\n'
                   'int main(void) {\n'
                   f'  size_t p[] = {{sizeof(urt_ReprojectDeform), {offs}}};\n'
                   '  for (unsigned k = 0; k < sizeof p / sizeof p[0]; k++) printf("%zu ", p[k]);\n'
                   '  printf("%g ", (double)URT_REPROJECT_DEFAULT_DEFORM_NORMAL_THRESHOLD);\n'
                   '  return fn == 0 || fc == 0;\n}\n')
    subprocess.run(["gcc", *inc, "-c", str(src), "-o", str(tmp_path / "layout.o")], check=True)     # compiles (linking needs the library)
    src2 = tmp_path / "sizes.c"
    src2.write_text(src.read_text().replace("= urt_reproject_deformed", "= 0").replace("= urt_buffer_copy", "= 0")
                    .replace("return fn == 0 || fc == 0;", "return fn != 0 || fc != 0;"))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", *inc, str(src2), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    p = [int(v) for v in out[:-1]]
    assert p[0] == C.sizeof(_lib.ReprojectDeform) == 40
    assert p[1:] == [getattr(_lib.ReprojectDeform, f).offset for f in DEFORM_FIELDS] == [0, 8, 16, 24, 32, 36]
    assert float(out[-1]) == _lib.REPROJECT_DEFORM_NORMAL_THRESHOLD


def test_symbols_are_declared_exported_and_in_the_csharp_binding(built_library):
    text = open(os.path.join(ROOT, "include", "urt.h")).read()
    assert re.search(r"URT_API int urt_reproject_deformed\(urt_context\* ctx, const urt_ReprojectImages\* images, const urt_ReprojectParams\* params,"
                     r"\s*const urt_ReprojectMotion\* motion[^,]*, const urt_ReprojectDeform\* deform[^)]*\);", text)
    assert re.search(r"URT_API int urt_buffer_copy\(urt_context\* ctx, urt_handle src, int src_first, urt_handle dst, int dst_first, int count\);", text)
    lib = C.CDLL(built_library)
    cs = open(os.path.join(ROOT, "integration", "UrtNative.cs")).read()
    shim = open(os.path.join(ROOT, "integration", "UrtUnityShim.cs")).read()
    for n in ("urt_reproject_deformed", "urt_buffer_copy"):
        assert n in _lib.ABI_SYMBOLS and hasattr(lib, n), n
        assert re.search(rf"\[DllImport\(Lib\)\]\s+internal static extern int {n}\(", cs), n
    m = re.search(r"internal struct ReprojectDeform \{(.*?)\n    \}", cs, re.S)
    assert m and re.findall(r"public (ulong|float|int) ([\w, ]+);", m.group(1)) == [("ulong", "prevVertices, indices, prevMeshObjects, deformed"),
                                                                                   ("float", "normalThreshold"), ("int", "flags")]
    assert re.search(r"public static void DeformMeshes\([^)]*bool keepHistory", shim) and "urt_reproject_deformed(ctx, in im, in p, in mo, in de)" in shim
    assert "urt_buffer_copy(ctx," in shim
    assert _lib.load().urt_abi_version() == 4


def test_null_context_is_rejected_without_a_device(built_library):
    lib = _lib.load()
    im, p, mo, de = _lib.ReprojectImages(*range(1, 12)), _lib.ReprojectParams(), _lib.ReprojectMotion(), _lib.ReprojectDeform(1, 2, 3, 4, 0.5, 0)
    assert lib.urt_reproject_deformed(None, C.byref(im), C.byref(p), C.byref(mo), C.byref(de)) == 1   # URT_ERR_INVALID_ARGUMENT
    assert lib.urt_reproject_deformed(None, C.byref(im), C.byref(p), None, None) == 1
    assert lib.urt_buffer_copy(None, 1, 0, 2, 0, 1) == 1


# ---- 2. the Python wrappers, on a stub library ---------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def urt_reproject(self, *a):
        self.calls.append(("reproject",))
        return 0

    def urt_reproject_objects(self, ctx, im, p, mo):
        self.calls.append(("reproject_objects", mo._obj.mesh_motion))
        return 0

    def urt_reproject_deformed(self, ctx, im, p, mo, de):
        m, d = mo._obj, de._obj
        self.calls.append(("reproject_deformed", m.mesh_motion, m.sphere_motion, m.moved_max_history,
                           d.prev_vertices, d.indices, d.prev_mesh_objects, d.deformed, d.normal_threshold, d.flags))
        return 0

    def urt_buffer_copy(self, ctx, src, src_first, dst, dst_first, count):
        self.calls.append(("buffer_copy", src, src_first, dst, dst_first, count))
        return 0


def stub_context():
    ctx = object.__new__(unity_api.Context)
    ctx.lib = _StubLib()
    ctx._h = C.c_void_p(1)
    ctx.device = 0
    return ctx


def stub_texture(ctx, handle, w=4, h=3):
    t = object.__new__(unity_api.RenderTexture)
    t.ctx, t.handle, t.width, t.height = ctx, handle, w, h
    return t


def stub_buffer(ctx, handle, count=3, stride=48):
    b = object.__new__(unity_api.ComputeBuffer)
    b.ctx, b.handle, b.count, b.stride = ctx, handle, count, stride
    return b


def reproject_kwargs(ctx):
    kw = {n: stub_texture(ctx, 11 + k) for k, n in enumerate(IMAGE_FIELDS)}
    kw["prev_world_to_clip"] = np.eye(4, dtype=F).reshape(16)
    return kw


def good_deform(ctx, **change):
    d = dict(prev_vertices=stub_buffer(ctx, 80, 10, 12), indices=stub_buffer(ctx, 81, 9, 4), prev_mesh_objects=stub_buffer(ctx, 82, 3, 112),
             deformed=stub_buffer(ctx, 83, 3, 4))
    d.update(change)
    return tuple(d.values())


DEFORM_BAD = {
    "not_a_tuple": (TypeError, lambda c: 5),
    "three_items": (ValueError, lambda c: good_deform(c)[:3]),
    "six_items": (ValueError, lambda c: good_deform(c) + (0.5, 0)),
    "array_for_a_buffer": (TypeError, lambda c: good_deform(c, prev_vertices=np.zeros((4, 3), F))),
    "texture_for_a_buffer": (TypeError, lambda c: good_deform(c, deformed=stub_texture(c, 5))),
    "other_context": (ValueError, lambda c: good_deform(c, indices=stub_buffer(stub_context(), 81, 9, 4))),
    "released": (ValueError, lambda c: good_deform(c, prev_mesh_objects=stub_buffer(c, 0, 3, 112))),
    "vertex_stride": (ValueError, lambda c: good_deform(c, prev_vertices=stub_buffer(c, 80, 10, 16))),
    "index_stride": (ValueError, lambda c: good_deform(c, indices=stub_buffer(c, 81, 9, 12))),
    "object_stride": (ValueError, lambda c: good_deform(c, prev_mesh_objects=stub_buffer(c, 82, 3, 48))),
    "flag_stride": (ValueError, lambda c: good_deform(c, deformed=stub_buffer(c, 83, 3, 8))),
    "indices_not_triangles": (ValueError, lambda c: good_deform(c, indices=stub_buffer(c, 81, 10, 4))),
    "counts_differ": (ValueError, lambda c: good_deform(c, deformed=stub_buffer(c, 83, 4, 4))),
    "threshold_nan": (ValueError, lambda c: good_deform(c) + (float("nan"),)),
    "threshold_str": (TypeError, lambda c: good_deform(c) + ("0.5",)),
}


@pytest.mark.parametrize("case", sorted(DEFORM_BAD))
def test_wrapper_rejects_bad_deform_arguments_before_the_library(case):
    exc, make = DEFORM_BAD[case]
    ctx = stub_context()
    with pytest.raises(exc):
        ctx.reproject(**reproject_kwargs(ctx), deform=make(ctx))
    assert ctx.lib.calls == []


def test_any_deform_makes_the_call_reproject_deformed():
    ctx = stub_context()
    ctx.reproject(**reproject_kwargs(ctx))
    ctx.reproject(**reproject_kwargs(ctx), mesh_motion=stub_buffer(ctx, 70), deform=None)
    ctx.reproject(**reproject_kwargs(ctx), deform=good_deform(ctx))
    ctx.reproject(**reproject_kwargs(ctx), deform=good_deform(ctx) + (-0.25,), mesh_motion=stub_buffer(ctx, 70), moved_max_history=8)

    class Holder:
        pass
    h = Holder()
    h.prev_vertices, h.indices, h.prev_mesh_objects, h.deformed = good_deform(ctx)
    ctx.reproject(**reproject_kwargs(ctx), deform=h, sphere_motion=stub_buffer(ctx, 71))
    h.normal_threshold = 0.75
    ctx.reproject(**reproject_kwargs(ctx), deform=h)
    d = float(np.float32(_lib.REPROJECT_DEFORM_NORMAL_THRESHOLD))                # as a C float holds it
    assert ctx.lib.calls == [("reproject",), ("reproject_objects", 70),
                             ("reproject_deformed", 0, 0, 0.0, 80, 81, 82, 83, d, 0), ("reproject_deformed", 70, 0, 8.0, 80, 81, 82, 83, -0.25, 0),
                             ("reproject_deformed", 0, 71, 0.0, 80, 81, 82, 83, d, 0), ("reproject_deformed", 0, 0, 0.0, 80, 81, 82, 83, 0.75, 0)]
    with pytest.raises(TypeError):
        ctx.reproject(**reproject_kwargs(ctx), deform=Holder())                # an object without the four attributes
    images = [np.zeros((3, 4, 4), F)] * 8
    eye = np.eye(4).reshape(16)
    for bad in ((np.zeros((4, 2), F), np.zeros(3, np.int32), np.zeros((1, 28), F), np.zeros(1, np.int32)),
                (np.zeros((0, 3), F), np.zeros(3, np.int32), np.zeros((1, 28), F), np.zeros(1, np.int32)),
                (np.zeros((4, 3), F), np.zeros(3, np.int32), np.zeros((1, 27), F), np.zeros(1, np.int32)),
                (np.zeros((4, 3), F), np.zeros(3, np.int32), np.zeros((1, 28), F)), 7):
        with pytest.raises(ValueError):
            ctx.reproject_arrays(*images, eye, eye, eye, deform=bad)


def test_copy_from_checks_its_arguments_before_the_library():
    ctx = stub_context()
    a, b = stub_buffer(ctx, 5, 10, 12), stub_buffer(ctx, 6, 20, 12)
    b.CopyFrom(a)
    b.CopyFrom(a, 2, 7, 3)
    b.CopyFrom(a, src_first=4)
    assert ctx.lib.calls == [("buffer_copy", 5, 0, 6, 0, 10), ("buffer_copy", 5, 2, 6, 7, 3), ("buffer_copy", 5, 4, 6, 0, 6)]
    ctx.lib.calls.clear()
    for exc, args in ((TypeError, (np.zeros(3),)), (TypeError, (a, 1.5)), (TypeError, (a, 0, True)), (TypeError, (a, 0, 0, "3")),
                      (ValueError, (stub_buffer(stub_context(), 5, 10, 12),))):
        with pytest.raises(exc):
            b.CopyFrom(*args)
    assert ctx.lib.calls == []


def test_keep_history_is_a_keyword_of_both_deformations_and_off_by_default():
    for fn in (RayTraceMaster.DeformMeshes, RayTraceMaster.SkinMeshes):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "keep_history" and p["keep_history"].default is False, fn.__name__
