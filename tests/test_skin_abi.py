"""The entry points of the device side of the buffers (include/urt.h urt_buffer_set_data_device, urt_buffer_get_data_range,
urt_skin_vertices, urt_buffer_bounds, urt_debug_buffer_state) exist, are declared in every binding and refuse a NULL context, and
RayTraceMaster.AttachSkin / SkinMeshes check their arguments before anything reaches the library.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_deform_abi import untouchable_context
from unityraytracer_amd import RayTraceMaster, _lib, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1
SYMBOLS = ("urt_buffer_set_data_device", "urt_buffer_get_data_range", "urt_skin_vertices", "urt_buffer_bounds", "urt_debug_buffer_state")


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_five_symbols_are_exported_and_declared_everywhere(built_library):
    lib = _lib.load()
    header, native = text("include", "urt.h"), text("integration", "UrtNative.cs")
    for name in SYMBOLS:
        assert getattr(lib, name) is not None and name in _lib.ABI_SYMBOLS, name
        assert re.search(r"URT_API int " + name + r"\(", header), name
        assert re.search(r"static extern int " + name + r"\(", native), name
    assert "urt_group_buffer_set_data_device" not in header and "urt_group_context" in header      # group twins: out of scope, and said so
    shim = text("integration", "UrtUnityShim.cs")
    assert "class UrtSkinnedMesh" in shim and "AttachSkin(" in shim and "SkinMeshes(" in shim


def test_layout_and_version(built_library):
    lib = _lib.load()
    assert C.sizeof(_lib.SkinBuffers) == 40
    assert [n for n, _ in _lib.SkinBuffers._fields_] == ["rest_vertices", "rest_normals", "bone_indices", "bone_weights", "bones"]
    assert re.search(r"urt_handle rest_vertices, rest_normals, bone_indices, bone_weights, bones;", text("include", "urt.h"))
    assert lib.urt_abi_version() == 4


def test_new_entry_points_refuse_a_null_context(built_library):
    lib = _lib.load()
    data = (C.c_float * 6)()
    out4 = (C.c_uint64 * 4)()
    n = C.c_int()
    sb = _lib.SkinBuffers(1, 2, 3, 4, 5)
    assert lib.urt_buffer_set_data_device(None, 1, 0, data, 1) == INVALID_ARGUMENT
    assert lib.urt_buffer_get_data_range(None, 1, 0, data, 1) == INVALID_ARGUMENT
    assert lib.urt_skin_vertices(None, C.byref(sb), 0, 1, 6, 7) == INVALID_ARGUMENT
    assert lib.urt_buffer_bounds(None, 1, 0, 1, data, C.byref(n)) == INVALID_ARGUMENT
    assert lib.urt_debug_buffer_state(None, 1, out4) == INVALID_ARGUMENT


def test_skin_calls_check_their_arguments_before_touching_a_context(built_library):
    sc = scenes.mixed_test_scene(96, 64)
    m = RayTraceMaster(untouchable_context(), sc)
    nb = 12 * 8 + 2
    idx, wgt = np.zeros((nb, 4), np.int32), np.zeros((nb, 4), np.float32)
    for key in ("0", 0.0, True, None):
        with pytest.raises(TypeError):
            m.AttachSkin(key, idx, wgt)
    for key in (-1, 3):
        with pytest.raises(IndexError):
            m.AttachSkin(key, idx, wgt)
    for bad in (idx[:-1], idx[:, :3], idx.reshape(-1), "indices", None):
        with pytest.raises(ValueError):
            m.AttachSkin(0, bad, wgt)
        with pytest.raises(ValueError):
            m.AttachSkin(0, idx, bad)
    with pytest.raises(ValueError):
        m.AttachSkin(2, idx, wgt)                                                  # the quad's span is 4 vertices
    m.AttachSkin(0, idx, wgt)
    assert np.array_equal(m._skins[0]["rest_vertices"], sc.vertices[:nb]) and m._skins[0]["span"] == (0, nb - 1)
    bones = np.zeros((2, 12), np.float32)
    with pytest.raises(TypeError):
        m.SkinMeshes({"0": bones})
    with pytest.raises(IndexError):
        m.SkinMeshes({7: bones})
    with pytest.raises(ValueError):
        m.SkinMeshes({1: bones})                                                   # no skin attached
    for bad in (bones[:, :11], bones.reshape(-1), bones[:0], "bones", None):
        with pytest.raises(ValueError):
            m.SkinMeshes({0: bad})
    with pytest.raises(TypeError):
        m.SkinMeshes(7)
