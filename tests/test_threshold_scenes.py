"""CPU: the scenes of tests/threshold_scenes.py have exactly the table sizes their cases name, and the oracle alone says that they are worth
rendering: the primitive kind a case is about is the first hit of a fifth of the pixels, nine objects in ten are the first hit of a
pixel, and so is the highest-numbered object — the one that exists only beyond the threshold."""
import numpy as np
import pytest

import lbvh_ref as L
import threshold_scenes as T
from oracle import pyoracle


def single_leaf_triangles(sc, leaf_max):
    """Triangles in MeshObjects whose whole triangle BVH is one leaf, by the restated host builder (tests/lbvh_ref.py build_sah)."""
    root = L.build_sah(sc, leaf_max)["mesh_root"]
    leaf = root[(root < 0)]
    return int(L.leaf_range(leaf)[1].sum()) if len(leaf) else 0, root


@pytest.mark.parametrize("name", list(T.CASES))
def test_sizes_are_the_ones_the_case_names(name):
    make, n_meshes, n_spheres, mesh_nodes, sphere_nodes, n_small, leaf_max = T.CASES[name]
    sc = make()
    assert (len(sc.mesh_objects), len(sc.spheres)) == (n_meshes, n_spheres)
    assert (len(sc.mesh_bvh), len(sc.sphere_bvh)) == (mesh_nodes, sphere_nodes)
    assert (T.heap_nodes(n_meshes), T.heap_nodes(n_spheres)) == (mesh_nodes, sphere_nodes)
    assert sc.width <= 128 and sc.height <= 80 and sc.num_bounces == 4 and sc.sky.shape[:2] == (32, 64)
    small, root = single_leaf_triangles(sc, leaf_max)
    assert small == n_small
    if n_small == 0:
        assert (root >= 0).all() and (sc.mesh_objects["indices_count"] >= 60).all()      # none is single-leaf at any leaf size up to 8
    if name.endswith("+big"):
        big = np.flatnonzero(root >= 0)
        assert len(big) == 1 and 0 < big[0] < n_meshes - 1                               # single-leaf MeshObjects on both sides of it


def test_the_listed_sizes_straddle_every_threshold():
    """12 | 13 MeshObjects (listed FRONT), 31 | 63 mesh-heap nodes (masked FRONT), 255 | 511 nodes of either heap and 256 | 257 spheres
    (LDS tables), 64 | 66 and 64 | 72 single-leaf triangles (LDS copy), 1 | 2 MeshObjects (FRONT at all), 1 .. 5 for the rounding of
    the root table to float4s."""
    c = T.CASES
    assert [c[k][1] for k in ("m1", "m2", "m3", "m4", "m5", "m12", "m13", "m16", "m17", "m128", "m129")] == [1, 2, 3, 4, 5, 12, 13, 16, 17, 128, 129]
    assert (c["m16"][3], c["m17"][3], c["m128"][3], c["m129"][3]) == (31, 63, 255, 511)
    assert (c["s128"][4], c["s129"][4], c["m16+s129"][4], c["m3+s257"][4]) == (255, 511, 511, 1023) and c["m3+s257"][2] == 257
    assert (c["fans8+big"][5], c["fans9+big"][5], c["quads32"][5], c["quads33"][5], c["quads32+big"][5]) == (64, 72, 64, 66, 64)
    assert c["fans9+big"][1] <= 16 and c["fans9+big"][3] <= 31 and c["quads32"][3] == 63


@pytest.mark.parametrize("name", list(T.CASES))
def test_the_oracle_sees_every_object(name):
    make, n_meshes, n_spheres = T.CASES[name][:3]
    sc = make()
    kind, obj = T.first_hits(sc, pyoracle.Oracle(sc))
    px = kind.size
    relevant = 2 if n_spheres else 3
    share = (kind == relevant).sum() / px
    print(f"{name}: sky {np.mean(kind == 0):.2f} ground {np.mean(kind == 1):.2f} sphere {np.mean(kind == 2):.2f} triangle {np.mean(kind == 3):.2f}")
    assert share >= 0.20, (name, share)
    for k, n in ((3, n_meshes), (2, n_spheres)):
        if n == 0:
            assert not (kind == k).any()
            continue
        seen = np.unique(obj[kind == k])
        print(f"{name}: {len(seen)} of {n} objects of kind {k} are a first hit")
        assert len(seen) >= 0.9 * n, (name, k, len(seen), n)
        assert n - 1 in seen, (name, k)
    # the frame the GPU tests compare is not black and sees the same kinds (one frame of the literal walk, with counters)
    img, oc = pyoracle.Oracle(sc).render(mode=0, threads=8, counters=True)
    assert (oc["hit_tri"] > 0) == (n_meshes > 0) and (oc["hit_sphere"] > 0) == (n_spheres > 0) and oc["pixels"] == px
    assert np.isfinite(img).all() and (img[..., :3] > 0).any(axis=2).mean() > 0.5
    if n_meshes:
        # ... and the oracle's BVH mode, which the GPU tests compare with, is that literal walk bit for bit — also on a forest without a
        # single node (quads alone: every root is a leaf code)
        o = pyoracle.Oracle(sc)
        nodes = o.build_own_blas()[0]
        assert (len(nodes) == 0) == name.startswith("quads3") * (not name.endswith("+big"))
        assert np.array_equal(o.render(mode=1, threads=8).view(np.uint32), img.view(np.uint32))
