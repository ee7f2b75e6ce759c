"""The entry points of the object-level BVH on the device (include/urt.h urt_mesh_leaf_bounds_device, urt_sphere_leaf_bounds_device,
urt_build_object_bvh_device) exist, are declared in every binding and refuse a NULL context, and a RayTraceMaster with
device_object_heaps = True checks the arguments of MoveObjects / SkinMeshes before anything reaches the library.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_deform_abi import untouchable_context
from unityraytracer_amd import Context, RayTraceMaster, _lib, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1
SYMBOLS = ("urt_mesh_leaf_bounds_device", "urt_sphere_leaf_bounds_device", "urt_build_object_bvh_device")


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_three_symbols_are_exported_and_declared_everywhere(built_library):
    lib = _lib.load()
    header, native = text("include", "urt.h"), text("integration", "UrtNative.cs")
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert getattr(lib, name) is not None and name in _lib.ABI_SYMBOLS, name
        assert re.search(r"URT_API int " + name + r"\(", header), name
        assert re.search(r"static extern int " + name + r"\(", native), name
        assert re.search(r" T " + name + r"$", exported, re.M), name
    assert "the object-level BVH on the device" in header
    assert not re.search(r"urt_group_\w*(leaf_bounds|object_bvh)", header) and "urt_group_context" in header      # group twins: out of scope, and said so
    assert "RebuildObjectHeapsOnDevice(" in text("integration", "UrtUnityShim.cs")


def test_constants_and_version(built_library):
    lib = _lib.load()
    header = text("include", "urt.h")
    assert int(re.search(r"#define URT_OBJECT_BVH_DEVICE_MAX (\d+)", header).group(1)) == _lib.OBJECT_BVH_DEVICE_MAX == 1024
    assert int(re.search(r"#define URT_MESH_LEAF_BLOCKS (\d+)", header).group(1)) == _lib.MESH_LEAF_BLOCKS
    assert int(re.search(r"ObjectBvhDeviceMax = (\d+)", text("integration", "UrtNative.cs")).group(1)) == _lib.OBJECT_BVH_DEVICE_MAX
    assert lib.urt_abi_version() == 4


def test_new_entry_points_refuse_a_null_context(built_library):
    lib = _lib.load()
    assert lib.urt_mesh_leaf_bounds_device(None, 1, 2, 3, 4) == INVALID_ARGUMENT
    assert lib.urt_sphere_leaf_bounds_device(None, 1, 2) == INVALID_ARGUMENT
    assert lib.urt_build_object_bvh_device(None, 1, 2) == INVALID_ARGUMENT


def test_wrappers_check_their_arguments_before_touching_a_context(built_library):
    ctx = Context.__new__(Context)                                                 # no library handle: a call that got past the checks would fail on it
    for call, n in ((ctx.mesh_leaf_bounds, 4), (ctx.sphere_leaf_bounds, 2), (ctx.build_object_bvh, 2)):
        for bad in (None, 7, "buffer", np.zeros(3)):
            with pytest.raises(TypeError):
                call(*([bad] * n))


def test_a_master_with_device_heaps_checks_its_arguments_before_touching_a_context(built_library):
    assert RayTraceMaster.device_object_heaps is False                             # off by default
    sc = scenes.mixed_test_scene(96, 64)
    m = RayTraceMaster(untouchable_context(), sc)
    m.device_object_heaps = True
    eye = np.eye(4, dtype=np.float32)
    for key in ("0", 0.0, True, None):
        with pytest.raises(TypeError):
            m.MoveObjects(mesh_edits={key: eye})
        with pytest.raises(TypeError):
            m.MoveObjects(sphere_edits={key: ((0, 0, 0), 1.0)})
    for key in (-1, len(sc.mesh_objects)):
        with pytest.raises(IndexError):
            m.MoveObjects(mesh_edits={key: eye})
    for key in (-1, len(sc.spheres)):
        with pytest.raises(IndexError):
            m.MoveObjects(sphere_edits={key: ((0, 0, 0), 1.0)})
    for bad in (np.zeros(15, np.float32), "matrix", None):
        with pytest.raises((TypeError, ValueError)):
            m.MoveObjects(mesh_edits={0: bad})
    for bad in (((0, 0), 1.0), (0, 0, 0, 1.0), "sphere", None):
        with pytest.raises(ValueError):
            m.MoveObjects(sphere_edits={0: bad})
    nb = 12 * 8 + 2
    m.AttachSkin(0, np.zeros((nb, 4), np.int32), np.zeros((nb, 4), np.float32))
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
    m.SyncObjectHeaps()                                                            # nothing is behind: nothing to read
