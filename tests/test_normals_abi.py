"""The entry points of the normals on the device (include/urt.h urt_normals_plan_create, urt_normals_plan_info,
urt_normals_plan_release, urt_compute_normals, urt_debug_build_normals_plan) exist, are declared in every binding and refuse a NULL
context; the host code behind the plan (csrc/normals_plan.cpp, pure C++) runs clean under the address and undefined-behaviour
sanitizers as a stand-alone program.  No GPU."""
import ctypes as C
import os
import re
import subprocess

from unityraytracer_amd import NormalsPlan, RayTraceMaster, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1
SYMBOLS = ("urt_normals_plan_create", "urt_normals_plan_info", "urt_normals_plan_release", "urt_compute_normals", "urt_debug_build_normals_plan")


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_five_symbols_are_exported_and_declared_everywhere(built_library):
    lib = _lib.load()
    header, native = text("include", "urt.h"), text("integration", "UrtNative.cs")
    for name in SYMBOLS:
        assert getattr(lib, name) is not None and name in _lib.ABI_SYMBOLS, name
        assert re.search(r"URT_API int " + name + r"\(", header), name
        assert re.search(r"static extern int " + name + r"\(", native), name
    assert "urt_group_normals_plan_create" not in header and "urt_group_compute_normals" not in header      # group twins: out of scope
    shim = text("integration", "UrtUnityShim.cs")
    assert "class UrtNormalsPlan" in shim and "Compute(" in shim
    assert callable(NormalsPlan.compute) and callable(RayTraceMaster.RecomputeNormals)
    assert "normals.hip" in text("unityraytracer_amd", "build.py") and "normals_plan.cpp" in text("unityraytracer_amd", "build.py")


def test_layout_and_version(built_library, tmp_path):
    lib = _lib.load()
    assert C.sizeof(_lib.NormalsPlanInfo) == 32
    assert [n for n, _ in _lib.NormalsPlanInfo._fields_] == ["first", "count", "n_lists", "n_triangles", "n_entries", "max_valence", "device_bytes"]
    assert _lib.NormalsPlanInfo.device_bytes.offset == 24
    assert lib.urt_abi_version() == 4
    (tmp_path / "layout.c").write_text('#include <stddef.h>\n#include "urt.h"\n'
                                       'typedef char size_is_32[sizeof(urt_NormalsPlanInfo) == 32 ? 1 : -1];\n'
                                       'typedef char bytes_at_24[offsetof(urt_NormalsPlanInfo, device_bytes) == 24 ? 1 : -1];\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                    str(tmp_path / "layout.c")], check=True)


def test_new_entry_points_refuse_a_null_context(built_library):
    lib = _lib.load()
    h = C.c_uint64(77)
    info = _lib.NormalsPlanInfo()
    assert lib.urt_normals_plan_create(None, 1, 2, 0, 1, C.byref(h)) == INVALID_ARGUMENT and h.value == 77
    assert lib.urt_normals_plan_info(None, 1, C.byref(info)) == INVALID_ARGUMENT
    assert lib.urt_normals_plan_release(None, 1) == INVALID_ARGUMENT
    assert lib.urt_compute_normals(None, 1, 2) == INVALID_ARGUMENT


def test_the_plan_code_runs_clean_under_the_host_sanitizers(tmp_path):
    """csrc/normals_plan.cpp has no HIP in it: it is compiled with tests/normals_plan_main.cpp, a program with its own main, by
    g++ -fsanitize=address,undefined with the sanitizer runtimes linked statically, and that program is run in the environment as it
    is.  Nothing is loaded into this process."""
    exe = str(tmp_path / "normals_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror", os.path.join(ROOT, "tests", "normals_plan_main.cpp"),
                    os.path.join(ROOT, "unityraytracer_amd", "csrc", "normals_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "normals plans: ok" in run.stdout, run.stdout + run.stderr
