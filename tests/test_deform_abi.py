"""The entry points of the deformed-mesh path (include/urt.h urt_buffer_set_data_range, urt_group_buffer_set_data_range,
urt_debug_deform_stats, urt_debug_scene_cost) exist and refuse a NULL context, and RayTraceMaster.DeformMeshes checks its arguments
before anything reaches the library.  No GPU."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from unityraytracer_amd import RayTraceMaster, _lib, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1


def test_new_entry_points_refuse_a_null_context(built_library):
    lib = _lib.load()
    data = (C.c_float * 3)(1, 2, 3)
    out6 = (C.c_uint64 * 6)()
    out2 = (C.c_float * 2)()
    assert lib.urt_buffer_set_data_range(None, 1, 0, data, 1) == INVALID_ARGUMENT
    assert lib.urt_group_buffer_set_data_range(None, 1, 0, data, 1) == INVALID_ARGUMENT
    assert lib.urt_debug_deform_stats(None, out6) == INVALID_ARGUMENT
    assert lib.urt_debug_scene_cost(None, out2, 1) == INVALID_ARGUMENT
    assert lib.urt_abi_version() == 4


def test_options_are_listed_in_the_header():
    text = open(os.path.join(ROOT, "include", "urt.h")).read()
    for name in ('"refit"', '"refit_vertices"', '"refit_rebuild_pct"'):
        assert name in text, name
    shim = open(os.path.join(ROOT, "integration", "UrtUnityShim.cs")).read()
    assert "urt_buffer_set_data_range" in shim and "public static void DeformMeshes(" in shim


def untouchable_context():
    """Stands in for a Context: any use beyond keeping a reference raises."""
    class Untouchable(types.SimpleNamespace):
        def __getattr__(self, name):
            raise AssertionError(f"the context was touched ({name})")
    return Untouchable()


def test_deform_meshes_checks_its_arguments_before_touching_a_context(built_library):
    sc = scenes.mixed_test_scene(96, 64)
    m = RayTraceMaster(untouchable_context(), sc)
    before = sc.vertices.copy()
    blob = np.zeros((12 * 8 + 2, 3), np.float32)
    assert m.vertex_span(0) == (0, len(blob) - 1) and m.vertex_span(2) == (len(sc.vertices) - 4, len(sc.vertices) - 1)
    for key in ("0", 0.0, True, None, (0,)):
        with pytest.raises(TypeError):
            m.DeformMeshes({key: blob})
    for key in (-1, 3, 10 ** 6):
        with pytest.raises(IndexError):
            m.DeformMeshes({key: blob})
    for bad in (blob[:-1], blob.reshape(-1), blob[:, :2], np.zeros((len(blob), 4), np.float32), "positions", [[1, 2, 3], [4, 5]], None):
        with pytest.raises(ValueError):
            m.DeformMeshes({0: bad})
    with pytest.raises(ValueError):
        m.DeformMeshes({2: blob})                                                  # the quad's span is 4 vertices
    with pytest.raises(TypeError):
        m.DeformMeshes(7)
    assert np.array_equal(sc.vertices, before) and m.scene.vertices is sc.vertices   # nothing was written by the refused calls
