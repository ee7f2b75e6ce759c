"""The entry points of the blend shapes on the device (include/urt.h urt_morph_plan_create, urt_morph_plan_info, urt_morph_plan_release,
urt_morph_vertices, urt_debug_build_morph_plan) exist, are declared in every binding and refuse a NULL context; RayTraceMaster's
AttachBlendShapes / MorphMeshes check their arguments before anything reaches the library; the host code behind the plan
(csrc/morph_plan.cpp, pure C++) runs clean under the address and undefined-behaviour sanitizers as a stand-alone program.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_deform_abi import untouchable_context
from unityraytracer_amd import Context, MorphPlan, RayTraceMaster, _lib, host_scene, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1
SYMBOLS = ("urt_morph_plan_create", "urt_morph_plan_info", "urt_morph_plan_release", "urt_morph_vertices", "urt_debug_build_morph_plan")


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_five_symbols_are_exported_and_declared_everywhere(built_library):
    lib = _lib.load()
    header, native = text("include", "urt.h"), text("integration", "UrtNative.cs")
    for name in SYMBOLS:
        assert getattr(lib, name) is not None and name in _lib.ABI_SYMBOLS, name
        assert re.search(r"URT_API int " + name + r"\(", header), name
        assert re.search(r"static extern int " + name + r"\(", native), name
    assert "urt_group_morph" not in header                                         # group twins: out of scope
    shim = text("integration", "UrtUnityShim.cs")
    assert "blendShapeCount" in shim and "GetBlendShapeWeight" in shim and "GetBlendShapeFrameWeight" in shim and "In-between frames" in shim
    assert callable(Context.morph_plan) and callable(MorphPlan.morph) and callable(MorphPlan.info) and callable(MorphPlan.Release)
    assert callable(RayTraceMaster.AttachBlendShapes) and callable(RayTraceMaster.MorphMeshes) and callable(host_scene.morph_plan)
    assert "morph.hip" in text("unityraytracer_amd", "build.py") and "morph_plan.cpp" in text("unityraytracer_amd", "build.py")


def test_layout_and_version(built_library, tmp_path):
    lib = _lib.load()
    assert C.sizeof(_lib.MorphDelta) == 32 and C.sizeof(_lib.MorphPlanInfo) == 32 and np.dtype(_lib.MORPH_DELTA_DT).itemsize == 32
    assert [n for n, _ in _lib.MorphDelta._fields_] == ["vertex", "target", "dp", "dn"]
    assert (_lib.MorphDelta.dp.offset, _lib.MorphDelta.dn.offset) == (8, 20)
    assert [np.dtype(_lib.MORPH_DELTA_DT).fields[n][1] for n in ("vertex", "target", "dp", "dn")] == [0, 4, 8, 20]
    assert [n for n, _ in _lib.MorphPlanInfo._fields_] == ["first", "count", "n_targets", "n_entries", "max_valence", "n_touched", "device_bytes"]
    assert _lib.MorphPlanInfo.device_bytes.offset == 24 and _lib.MORPH_NORMALIZE == 1
    assert lib.urt_abi_version() == 4
    (tmp_path / "layout.c").write_text('#include <stddef.h>\n#include "urt.h"\n'
                                       'typedef char delta_is_32[sizeof(urt_MorphDelta) == 32 ? 1 : -1];\n'
                                       'typedef char dn_at_20[offsetof(urt_MorphDelta, dn) == 20 ? 1 : -1];\n'
                                       'typedef char info_is_32[sizeof(urt_MorphPlanInfo) == 32 ? 1 : -1];\n'
                                       'typedef char bytes_at_24[offsetof(urt_MorphPlanInfo, device_bytes) == 24 ? 1 : -1];\n'
                                       'typedef char normalize_is_1[URT_MORPH_NORMALIZE == 1 ? 1 : -1];\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                    str(tmp_path / "layout.c")], check=True)


def test_new_entry_points_refuse_a_null_context(built_library):
    lib = _lib.load()
    h = C.c_uint64(77)
    info = _lib.MorphPlanInfo()
    d = _lib.MorphDelta(0, 0)
    assert lib.urt_morph_plan_create(None, C.byref(d), 1, 1, 0, 1, C.byref(h)) == INVALID_ARGUMENT and h.value == 77
    assert lib.urt_morph_plan_info(None, 1, C.byref(info)) == INVALID_ARGUMENT
    assert lib.urt_morph_plan_release(None, 1) == INVALID_ARGUMENT
    assert lib.urt_morph_vertices(None, 1, 2, 3, 4, 5, 6, 0) == INVALID_ARGUMENT


def test_blend_shape_calls_check_their_arguments_before_touching_a_context(built_library):
    sc = scenes.mixed_test_scene(96, 64)
    m = RayTraceMaster(untouchable_context(), sc)
    nb = 12 * 8 + 2
    dp, dn = np.zeros((nb, 3), np.float32), np.zeros((nb, 3), np.float32)
    dp[3] = (1, 0, 0); dn[5] = (0, 0, 2); dp[7, 1] = -0.0                          # rows 3 and 5 stay; -0.0 == 0: row 7 is dropped
    for key in ("0", 0.0, True, None):
        with pytest.raises(TypeError):
            m.AttachBlendShapes(key, [(dp, dn)])
    for key in (-1, 3):
        with pytest.raises(IndexError):
            m.AttachBlendShapes(key, [(dp, dn)])
    for bad in (dp[:-1], dp[:, :2], dp.reshape(-1), "deltas", None):
        with pytest.raises(ValueError):
            m.AttachBlendShapes(0, [(bad, dn)])
        if bad is not None:                                                        # (None for the normals: no normal deltas)
            with pytest.raises(ValueError):
                m.AttachBlendShapes(0, [(dp, bad)])
    for bad in ([], "targets", None, 7, [dp], [(dp,)], [(dp, dn, dn)], [(dp, None)] * 4097):
        with pytest.raises(ValueError):
            m.AttachBlendShapes(0, bad)
    with pytest.raises(ValueError):
        m.AttachBlendShapes(2, [(dp, dn)])                                         # the quad's span is 4 vertices
    assert not m._morphs
    m.AttachBlendShapes(0, [(dp, dn), (dp * 2, None), (np.zeros_like(dp), None)])
    mp = m._morphs[0]
    assert np.array_equal(mp["rest_vertices"], sc.vertices[:nb]) and np.array_equal(mp["rest_normals"], sc.normals[:nb])
    assert mp["span"] == (0, nb - 1) and mp["n_targets"] == 3 and mp["plan"] is None
    d = mp["deltas"]
    assert d.dtype == np.dtype(_lib.MORPH_DELTA_DT) and d["vertex"].tolist() == [3, 5, 3] and d["target"].tolist() == [0, 0, 1]
    assert d["dp"].tolist() == [[1, 0, 0], [0, 0, 0], [2, 0, 0]] and d["dn"].tolist() == [[0, 0, 0], [0, 0, 2], [0, 0, 0]]
    quad = np.ones((4, 3), np.float32)
    m.AttachBlendShapes(2, [(quad, None)])                                         # absolute vertex numbers
    assert m._morphs[2]["deltas"]["vertex"].tolist() == list(range(len(sc.vertices) - 4, len(sc.vertices)))
    w = np.zeros(3, np.float32)
    with pytest.raises(TypeError):
        m.MorphMeshes({"0": w})
    with pytest.raises(IndexError):
        m.MorphMeshes({7: w})
    with pytest.raises(ValueError):
        m.MorphMeshes({1: w})                                                      # no blend shapes attached
    for bad in (w[:2], np.zeros(4, np.float32), w.reshape(3, 1), "weights", None, 1.0):
        with pytest.raises(ValueError):
            m.MorphMeshes({0: bad})
    with pytest.raises(TypeError):
        m.MorphMeshes(7)
    bones = np.zeros((2, 12), np.float32)
    with pytest.raises(ValueError):
        m.MorphMeshes({0: w}, poses={0: bones})                                    # no skin attached
    m.AttachSkin(0, np.zeros((nb, 4), np.int32), np.zeros((nb, 4), np.float32))
    m.AttachSkin(1, np.zeros((m.vertex_span(1)[1] - m.vertex_span(1)[0] + 1, 4), np.int32),
                 np.zeros((m.vertex_span(1)[1] - m.vertex_span(1)[0] + 1, 4), np.float32))
    with pytest.raises(ValueError):
        m.MorphMeshes({0: w}, poses={1: bones})                                    # a pose for a mesh that is not morphed
    with pytest.raises(ValueError):
        m.MorphMeshes({0: w}, poses={0: bones[:, :11]})
    with pytest.raises(TypeError):
        m.MorphMeshes({0: w}, poses={"0": bones})
    with pytest.raises(TypeError):
        m.MorphMeshes({0: w}, poses=7)


def test_the_plan_code_runs_clean_under_the_host_sanitizers(tmp_path):
    """csrc/morph_plan.cpp has no HIP in it: it is compiled with tests/morph_plan_main.cpp, a program with its own main, by
    g++ -fsanitize=address,undefined with the sanitizer runtimes linked statically, and that program is run in the environment as it
    is.  Nothing is loaded into this process."""
    exe = str(tmp_path / "morph_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror", os.path.join(ROOT, "tests", "morph_plan_main.cpp"),
                    os.path.join(ROOT, "unityraytracer_amd", "csrc", "morph_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "morph plans: ok" in run.stdout, run.stdout + run.stderr
