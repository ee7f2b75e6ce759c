"""The oracle's radiance probe (oracle_probe_radiance / pyoracle.radiance): the URT_RADIANCE_RAYS paragraph of include/urt.h restated
over the Tracer's own Trace and Shade.  Pinned here, without a GPU, against the oracle's literal render, its sky lookup and the
materials' emission, so that tests/test_gpu_radiance_rays.py can take it as the reference for arbitrary rays."""
import numpy as np

from oracle import pyoracle
from unityraytracer_amd import scenes

from test_gpu_aov import camera_rays

F = np.float32
W, H = 40, 24
POX, POY, SEED = 0.3125, 0.71875, 0.4375


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def frame_rays(sc):
    """The first ray of every pixel of a 1-ray frame with (_PixelOffset, _Seed) = (POX, POY), SEED, as urt_PathRay records: the seed
    after the two jitter draws, px/py = the pixel."""
    O, D = camera_rays(sc, W, H, frame=(POX, POY, SEED))
    X, Y = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    seed_after = F(F(F(SEED) + F(0.5)) + F(0.5))
    return pyoracle.path_rays(O.reshape(-1, 3), D.reshape(-1, 3), np.stack([X.reshape(-1), Y.reshape(-1)], axis=1), seed_after)


def test_probe_equals_the_literal_render():
    sc = scenes.mixed_test_scene(W, H)
    sc.num_rays, sc.num_bounces = 1, 4
    orc = pyoracle.Oracle(sc)
    orc.set_frame((POX, POY), SEED)
    ref = orc.render(mode=0, threads=4).reshape(-1, 4)
    got = pyoracle.radiance(orc, frame_rays(sc), 1, 4, mode=0)
    assert np.array_equal(bits(got), bits(ref))
    assert (ref[:, :3] > 0).any(axis=1).mean() > 0.9                 # the frame is lit


def test_the_seed_carries_over_between_samples():
    """Two samples of a ray are the one-sample queries from the seed the first path left behind: different paths, and their float32
    mean.  (A probe that reset the seed per sample would return the first sample twice.)"""
    sc = scenes.mixed_test_scene(W, H)
    orc = pyoracle.Oracle(sc)
    rays = frame_rays(sc)
    one = pyoracle.radiance(orc, rays, 1, 4)
    two = pyoracle.radiance(orc, rays, 2, 4)
    differ = (bits(one) != bits(two)).any(axis=1)
    # a path that ends on the sky at once draws nothing: its second sample repeats the first exactly, and the mean is the value itself
    miss = np.array([orc.trace(r[0:3], r[4:7])["kind"] == 0 for r in rays])
    assert miss.sum() > 50 and not differ[miss].any()
    # a path that hits something draws its roulette from the seed: with the seed carried over the second path is another one, unless
    # both end absorbed with the same light.  With the seed reset per sample no query at all would differ.
    assert (~miss).sum() > 50 and differ[~miss].mean() > 0.5


def test_zero_bounces_give_black_with_alpha_one():
    sc = scenes.mixed_test_scene(W, H)
    got = pyoracle.radiance(pyoracle.Oracle(sc), frame_rays(sc)[:70], 3, 0)
    assert np.array_equal(got, np.tile(np.array([0, 0, 0, 1], F), (70, 1)))


def test_a_miss_is_the_mean_of_three_sky_lookups_in_float32():
    sc = scenes.mixed_test_scene(W, H, sky=np.random.default_rng(2).random((19, 37, 4)).astype(F))
    orc = pyoracle.Oracle(sc)
    rng = np.random.default_rng(3)
    D = rng.normal(size=(64, 3))
    D[:, 1] = np.abs(D[:, 1]) + 0.05                                 # upwards from above the scene: nothing to hit
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(F)
    O = np.tile(np.array([0, 50, 0], F), (64, 1))
    assert all(orc.trace(o, d)["kind"] == 0 for o, d in zip(O, D))
    got = pyoracle.radiance(orc, pyoracle.path_rays(O, D, rng.random((64, 2)) * 100, 0.25), 3, 4)
    s = np.stack([orc.sky(d) for d in D])
    want = (((s + s).astype(F) + s).astype(F) / F(3)).astype(F)      # avg = ((0 + s) + s) + s, then / (float)samples
    assert np.array_equal(bits(got[:, :3]), bits(want)) and (got[:, 3] == 1).all()
    assert (bits(want) != bits(s)).any()                             # and that is not s itself: the order of the sums shows


def test_one_bounce_at_the_emissive_quad_is_its_emission():
    sc = scenes.mixed_test_scene(W, H)
    orc = pyoracle.Oracle(sc)
    gx, gz = np.meshgrid(np.linspace(-1.3, 1.3, 4), np.linspace(-0.3, 2.3, 4))
    below = np.stack([gx.reshape(-1), np.full(16, 3.0), gz.reshape(-1)], axis=1)
    O = np.concatenate([below, below + np.array([0, 1.0, 0])])
    D = np.concatenate([np.tile([0, 1, 0], (16, 1)), np.tile([0, -1, 0], (16, 1))])
    got = pyoracle.radiance(orc, pyoracle.path_rays(O, D, np.zeros((32, 2)), 0.25), 2, 1)
    em = sc.mesh_objects["lighting"]["emission"]
    quad = int(np.argmax(em.sum(axis=1)))
    assert (em[quad] == np.array([6, 5, 4], F)).all()
    hit = [orc.trace(o, d) for o, d in zip(O, D)]
    facing = np.array([h["kind"] == 3 and abs(h["position"][1] - 3.5) < 1e-3 for h in hit])
    assert facing[:16].all() != facing[16:].all() and facing.sum() == 16     # one side of the quad faces its rays, the other is culled
    assert np.array_equal(bits(got[facing, :3]), bits(np.tile(em[quad], (16, 1))))


def test_the_answer_does_not_depend_on_the_thread_count():
    sc = scenes.mixed_test_scene(W, H)
    orc = pyoracle.Oracle(sc)
    rays = frame_rays(sc)[:333]
    one = pyoracle.radiance(orc, rays, 2, 4, threads=1)
    for threads in (2, 7, 16, 500):
        assert np.array_equal(bits(pyoracle.radiance(orc, rays, 2, 4, threads=threads)), bits(one)), threads
    assert np.array_equal(bits(pyoracle.radiance(orc, rays, 2, 4)), bits(one))
    assert pyoracle.radiance(orc, rays[:0], 2, 4).shape == (0, 4)
