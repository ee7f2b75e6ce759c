"""The entry points and the option of the device-fed full preparation (include/urt.h option "prepare_device",
urt_debug_scene_vertex_spans, urt_debug_prepare_stats) are declared, bound and documented, and RayTraceMaster.ReplaceGeometryDevice
checks its arguments before anything reaches the library.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_deform_abi import untouchable_context
from unityraytracer_amd import RayTraceMaster, _lib, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1
NAMES = ("urt_debug_scene_vertex_spans", "urt_debug_prepare_stats")


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_header_declares_the_entry_points():
    text = read("include", "urt.h")
    assert re.search(r"URT_API int urt_debug_scene_vertex_spans\(urt_context\* ctx, int32_t\* out_lo, int32_t\* out_hi, int n_meshes\);", text)
    assert re.search(r"URT_API int urt_debug_prepare_stats\(urt_context\* ctx, uint64_t out4\[4\]\);", text)
    assert "URT_ABI_SIGN * 4" in read("unityraytracer_amd", "csrc", "context.cpp")          # additive: the ABI version stays


def test_the_binding_and_the_csharp_file_list_them(built_library):
    lib = _lib.load()
    cs = read("integration", "UrtNative.cs")
    for name in NAMES:
        assert name in _lib.ABI_SYMBOLS and getattr(lib, name) is not None, name
        assert re.search(r"\[DllImport\(Lib\)\]\s+internal static extern int " + name + r"\(", cs), name
    lo, hi, out4 = (C.c_int32 * 1)(), (C.c_int32 * 1)(), (C.c_uint64 * 4)()
    assert lib.urt_debug_scene_vertex_spans(None, lo, hi, 1) == INVALID_ARGUMENT
    assert lib.urt_debug_prepare_stats(None, out4) == INVALID_ARGUMENT
    assert lib.urt_abi_version() == 4


def test_the_option_is_documented():
    text = read("include", "urt.h")
    assert '"prepare_device" (0/1, default 0' in text
    options = text[text.index('"refit_vertices" (0/1'):text.index("URT_API int urt_set_option")]
    assert '"prepare_device"' in options                                        # in the option list, next to refit_vertices
    assert "sees the device-written data through the download.\n" not in text  # the promise that EVERY full preparation downloads is gone
    assert '{"prepare_device", &O::prepare_device' in read("unityraytracer_amd", "csrc", "context.cpp")
    shim = read("integration", "UrtUnityShim.cs")
    assert "public void ReplaceGeometryDevice(" in shim and '"prepare_device"' in shim
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "prepare_device" in read(doc), doc


def test_replace_geometry_device_checks_its_arguments_before_touching_a_context(built_library):
    sc = scenes.mixed_test_scene(96, 64)
    m = RayTraceMaster(untouchable_context(), sc)
    assert m.device_prepare is False
    dev = (0x1000, 8)
    with pytest.raises(ValueError):
        m.ReplaceGeometryDevice(dev, dev, dev, sc.mesh_objects)                   # no heap, and none can be built on the device
    for bad in (np.zeros(3, np.float32), "records", sc.mesh_objects.reshape(1, -1)):
        with pytest.raises(ValueError):
            m.ReplaceGeometryDevice(dev, dev, dev, bad, sc.mesh_bvh)
    with pytest.raises(ValueError):
        m.ReplaceGeometryDevice(dev, dev, dev, sc.mesh_objects, np.zeros(7, np.float32))
    for bad in (None, 0x1000, (0x1000,), [0x1000, 8], np.zeros((4, 3), np.float32)):
        with pytest.raises(TypeError):
            m.ReplaceGeometryDevice(bad, dev, dev, sc.mesh_objects, sc.mesh_bvh)
    for bad in ((0x1000, 2.0), ("a", 3), (True, 3)):
        with pytest.raises(TypeError):
            m.ReplaceGeometryDevice(dev, bad, dev, sc.mesh_objects, sc.mesh_bvh)
    for bad in ((0x1000, -1), (0x1000, 0)):
        with pytest.raises(ValueError):
            m.ReplaceGeometryDevice(dev, dev, bad, sc.mesh_objects, sc.mesh_bvh)
    assert m.scene.mesh_objects is sc.mesh_objects and m._vertexBuffer is None      # nothing was written by the refused calls
