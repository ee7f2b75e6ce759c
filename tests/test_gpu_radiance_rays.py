"""GPU: radiance queries of arbitrary rays (include/urt.h urt_radiance_query, URT_RADIANCE_RAYS) against the oracle's literal restatement
(pyoracle.radiance, mode 0: brute force over every triangle and sphere, pinned by tests/test_oracle_radiance.py), bit for bit, NaN equal
to NaN — probes inside the scenes with directions over the whole sphere, directed and unnormalised rays, the sky's wrap edges, random
streams outside a frame's, the ends of the sample and bounce ranges, batch sizes around a wave and a workgroup — each with both kernels
(radiance_persist 0 / 1) — and the resident-grid kernel on batches of more than twice the lanes the chip can hold, so that most queries
are taken by a lane that has finished another one, in rays mode and in pixels mode with runs of refused pixels.

Finite inputs only: with a NaN or an infinity in a ray the oracle's (int) conversions (f_sincos, the sky's texel index) are undefined
on the host, so there is nothing to compare with."""
import copy

import numpy as np
import pytest

from oracle import pyoracle
from unityraytracer_amd import Context, RayTraceMaster, scenes

from test_gpu_aov import bind, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 40, 24
THREADS = 16                                                         # of the oracle; never sized by the machine's CPU count


def cornell_scene():
    """C4 in small: Cornell box + 3 blobs = 9 MeshObjects, the masked object-level walk."""
    return scenes.config4(W, H, slices=24, stacks=19, sky=scenes.make_sky(64, 32))


SCENES = {"mixed": lambda: scenes.mixed_test_scene(W, H),
          "spheres": lambda: scenes.config2(W, H, sky=scenes.make_sky(37, 19)),
          "cornell": cornell_scene}
KINDS = {"mixed": (0, 1, 2, 3), "spheres": (0, 1, 2), "cornell": (0, 1, 3)}      # miss, ground, sphere, triangle
BOX = {"mixed": ((-4, 0.05, -4), (4, 4.5, 4)), "spheres": ((-4, 0.05, -4), (4, 4.5, 4)), "cornell": ((-4.5, 0.05, -4.5), (4.5, 9.5, 4.5))}


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    """A context of this module's own: no buffers of another module's scene stay bound, and its options start at their defaults."""
    with Context(gpu_ctx.device) as c:
        yield c


class Bound:
    """A scene bound to the context, with its oracle."""

    def __init__(self, ctx, sc):
        self.ctx, self.sc = ctx, sc
        self.m = bind(ctx, sc)
        self.orc = pyoracle.Oracle(sc)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.set_option("radiance_persist", -1)
        self.m.OnDisable()

    def query(self, rays, samples, bounces, persist, device=False):
        """urt_radiance_query(_device) over urt_PathRay records (n, 12) with the chosen kernel."""
        O, D, P, S = (np.ascontiguousarray(a) for a in (rays[:, 0:3], rays[:, 4:7], rays[:, 8:10], rays[:, 3]))
        self.ctx.set_option("radiance_persist", persist)
        try:
            if device:
                import torch
                dev = torch.device("cuda", self.ctx.device)
                t = lambda a: torch.from_numpy(a).to(dev)            # noqa: E731
                return self.ctx.radiance_query(t(O), t(D), t(P), t(S), samples, bounces).cpu().numpy()
            return self.ctx.radiance_query(O, D, P, S, samples, bounces)
        finally:
            self.ctx.set_option("radiance_persist", -1)

    def oracle(self, rays, samples, bounces):
        return pyoracle.radiance(self.orc, rays, samples, bounces, mode=0, threads=THREADS)

    def kinds(self, rays):
        return self.ctx.ray_query(np.ascontiguousarray(rays[:, 0:3]), np.ascontiguousarray(rays[:, 4:7]))["kind"]


def equal(got, ref):
    return bool(same_bits(got, ref).all())


def where_differs(got, ref, rays):
    bad = np.nonzero(~same_bits(got, ref).all(axis=1))[0]
    return f"{len(bad)} of {len(ref)} differ; first: " + "; ".join(f"#{i} ray {rays[i].tolist()} got {got[i].tolist()} ref {ref[i].tolist()}"
                                                                    for i in bad[:3])


def probes(rng, n, box, seeds=(0.0, 1.0), pix=100.0):
    """n urt_PathRay records: origins uniform in the box, unit directions uniform on the sphere, seeds uniform in `seeds`, px, py in
    [0, pix)."""
    lo, hi = np.array(box[0]), np.array(box[1])
    O = lo + rng.random((n, 3)) * (hi - lo)
    D = rng.normal(size=(n, 3))
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    S = seeds[0] + rng.random(n) * (seeds[1] - seeds[0])
    return pyoracle.path_rays(O, D, rng.random((n, 2)) * pix, S)


# ---- B.1 probes inside the scene ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["mixed", "spheres", "cornell"])
def test_probes_inside_the_scene(ctx, scene):
    rays = probes(np.random.default_rng(1), 2048, BOX[scene])
    with Bound(ctx, SCENES[scene]()) as b:
        ref = b.oracle(rays, 3, 6)
        kind = b.kinds(rays)
        got = {p: b.query(rays, 3, 6, p) for p in (0, 1)}
        got["device"] = b.query(rays, 3, 6, 1, device=True)
    count = np.bincount(kind, minlength=4)
    print(scene, "first-hit kinds", count.tolist(), "lit", float((ref[:, :3] > 0).any(axis=1).mean()))
    assert all(count[k] >= 64 for k in KINDS[scene]) and count.sum() == sum(count[k] for k in KINDS[scene]), count
    assert (ref[:, :3] > 0).any(axis=1).mean() >= 0.9
    for p, g in got.items():
        assert equal(g, ref), (scene, p, where_differs(g, ref, rays))


# ---- B.2 directed rays ----------------------------------------------------------------------------------------------------------------
DIRECTIONS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (-0.0, 1, -0.0), (1e-30, 1, 1e-30), (1e-7, 0, 1),
              (-1e-7, 0, 1), (0, 0, 0)]


def special_origins(sc):
    """Points in free space, inside a sphere, inside the largest mesh, on and below the ground plane, and on the emitter's plane."""
    pts = [(0.3, 2.0, -3.0), (0.0, 6.0, 0.25), (-3.7, 0.6, 3.1),     # free space
           (0.7, 0.0, -1.9), (0.7, -1.0, -1.9)]                      # exactly on the ground, and below it
    if len(sc.spheres):
        k = int(np.argmax(sc.spheres["radius"]))
        c, r = sc.spheres["position"][k].astype(np.float64), float(sc.spheres["radius"][k])
        pts += [tuple(c), tuple(c + np.array([0.3, -0.2, 0.4]) * r)]                               # inside a sphere
    if len(sc.mesh_objects):
        mo = sc.mesh_objects[int(np.argmax(sc.mesh_objects["indices_count"]))]                     # the (largest) blob
        wv = scenes.world_vertices(mo, sc.vertices, sc.indices)
        pts += [tuple(wv.mean(axis=0))]                                                            # inside it: the blob is star-shaped
        em = sc.mesh_objects["lighting"]["emission"].sum(axis=1)
        qv = scenes.world_vertices(sc.mesh_objects[int(np.argmax(em))], sc.vertices, sc.indices)
        assert em.max() > 0 and np.ptp(qv[:, 1]) == 0
        pts += [tuple(qv.mean(axis=0)), tuple(qv.mean(axis=0) + np.array([0.4, 0, -0.3]))]         # on the emissive quad's plane
    return np.array(pts, F)


@pytest.mark.parametrize("scene", ["mixed", "spheres", "cornell"])
def test_directed_and_unnormalised_rays(ctx, scene):
    """Axis-parallel, nearly axis-parallel and zero directions from origins in free space, inside objects, on and under the ground
    and on the emitter's plane; every ray also with its direction scaled by 0.01 and by 100: directions are used as given.  NaN and
    infinities are out of scope (module docstring)."""
    sc = SCENES[scene]()
    P = special_origins(sc)
    O = np.repeat(P, len(DIRECTIONS) * 3, axis=0)
    D = np.tile(np.concatenate([np.array(DIRECTIONS, F) * F(s) for s in (1, 0.01, 100)]), (len(P), 1)).astype(F)
    rng = np.random.default_rng(21)
    rays = pyoracle.path_rays(O, D, rng.random((len(O), 2)) * 100, rng.random(len(O)))
    assert np.isfinite(rays).all() and (np.signbit(rays[:, 4]) & (rays[:, 4] == 0)).any()          # the -0.0 survived
    with Bound(ctx, sc) as b:
        ref = b.oracle(rays, 3, 6)
        got = {p: b.query(rays, 3, 6, p) for p in (0, 1)}
        culled = got[1]
        if not equal(culled, ref):                                   # tell the object-level cull apart from the rest
            ctx.set_option("front_cull", 0)
            try:
                plain = b.query(rays, 3, 6, 1)
            finally:
                ctx.set_option("front_cull", 1)
            print("front_cull = 0:", "equal" if equal(plain, ref) else where_differs(plain, ref, rays))
    print(scene, len(rays), "rays, lit", float((ref[:, :3] > 0).any(axis=1).mean()), "NaN", int(np.isnan(ref).any(axis=1).sum()))
    assert (ref[:, :3] > 0).any(axis=1).mean() > 0.5
    for p, g in got.items():
        assert equal(g, ref), (scene, p, where_differs(g, ref, rays))


# ---- B.3 the sky's edges --------------------------------------------------------------------------------------------------------------
def sky_directions():
    d = [np.array(DIRECTIONS, np.float64)]
    a = np.arange(720) * (2 * np.pi / 720)                           # a ring of azimuths, level and raised; a = 0 is d.x = +0, d.z > 0
    for y in (0.0, 0.3):
        d.append(np.stack([np.sin(a), np.full(720, y), np.cos(a)], axis=1))
    tiny = [(s * t, y, 1.0) for s in (1, -1) for t in (0.0, 1e-30, 1e-7) for y in (0.0, 0.5, -0.5)]      # phi = -+0.5: both ends of the wrap
    d.append(np.array(tiny))
    e = np.deg2rad(np.arange(-90, 91))                               # 181 elevations
    el = np.stack([0.6 * np.cos(e), np.sin(e), 0.8 * np.cos(e)], axis=1)
    el[0], el[-1] = (0, -1, 0), (0, 1, 0)                            # theta = -1 (leaves the fast wrap's range) and theta = 0, exactly
    d.append(el)
    d = np.concatenate(d).astype(F)
    return np.concatenate([d, d * F(0.01), d * F(100)])


@pytest.mark.parametrize("sky_w, sky_h", [(1, 1), (2, 1), (3, 5), (37, 19), (128, 64)])
def test_the_skys_edges(ctx, sky_w, sky_h):
    """One-bounce queries that miss everything return the sky lookup of their direction: skies of random texels (a wrong texel or a
    wrong weight shows), sizes that are no power of two and the smallest there are; directions at both ends of the azimuth's wrap
    (phi = -+0.5), straight up and straight down (theta = 0 and -1), unnormalised too."""
    sky = np.random.default_rng(100 * sky_w + sky_h).random((sky_h, sky_w, 4)).astype(F)
    sc = scenes.config1(W, H, sky=sky)
    D = sky_directions()
    O = np.where((D[:, 1] >= 0)[:, None], np.array([0, 50, 0], F), np.array([0, -1, 0], F)).astype(F)      # nothing above, nothing below
    rng = np.random.default_rng(31)
    rays = pyoracle.path_rays(O, D, rng.random((len(D), 2)) * 100, rng.random(len(D)))
    with Bound(ctx, sc) as b:
        assert (b.kinds(rays) == 0).all()                            # every one is a miss
        sky_ref = np.stack([b.orc.sky(d) for d in D])
        ref = b.oracle(rays, 1, 1)
        got = {p: b.query(rays, 1, 1, p) for p in (0, 1)}
    assert equal(ref[:, :3], sky_ref) and (ref[:, 3] == 1).all()
    assert len(np.unique(ref.view(np.uint32), axis=0)) >= min(sky_w * sky_h, 64)      # the lookups reach all over the texture
    for p, g in got.items():
        assert equal(g, ref), (sky_w, sky_h, p, where_differs(g, ref, rays))


# ---- B.4 random streams outside a frame's ---------------------------------------------------------------------------------------------
def test_random_streams_outside_a_frames(ctx):
    """px, py negative, fractional and up to +-4096, seeds zero, negative and up to 64 — inside the range where the query is defined:
    |a * d| * 0.6366 < 2^30 in rand_next (include/urt_types.h urt_PathRay), so that f_sincos's (int)k is defined on the host."""
    rng = np.random.default_rng(41)
    n, samples, bounces = 2048, 3, 6
    rays = probes(rng, n, BOX["mixed"])
    P = (rng.random((n, 2)) * 2 - 1) * 4096
    P[:64] = np.round(P[:64])                                        # whole numbers too
    P[64:72] = [(-4096, -4096), (4096, 4096), (-4096, 4096), (4096, -4096), (0, 0), (-0.0, -0.0), (-0.5, 0.25), (4095.75, -0.125)]
    S = (rng.random(n) * 2 - 1) * 64
    S[:8] = [0, -0.0, 64, -64, 0.5, -0.5, 63.999, -1e-3]
    rays[:, 8:10], rays[:, 3] = P, S
    draws = samples * bounces * 3                                    # per bounce: the roulette and SampleHemisphere's two
    a = (np.abs(rays[:, 3].astype(np.float64)) + 0.5 * draws) * (1 + 1 / 17) / 100
    d = np.abs(rays[:, 8].astype(np.float64)) * 12.9898 + np.abs(rays[:, 9].astype(np.float64)) * 78.233
    assert (a * d * 0.6366).max() < 2.0 ** 30
    with Bound(ctx, SCENES["mixed"]()) as b:
        ref = b.oracle(rays, samples, bounces)
        got = {p: b.query(rays, samples, bounces, p) for p in (0, 1)}
    assert (ref[:, :3] > 0).any(axis=1).mean() >= 0.9
    for p, g in got.items():
        assert equal(g, ref), (p, where_differs(g, ref, rays))


# ---- B.5 ranges and batch shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples, bounces", [(4096, 1), (1, 64)])
def test_the_ends_of_the_ranges(ctx, samples, bounces):
    rays = probes(np.random.default_rng(51), 64, BOX["mixed"])
    with Bound(ctx, SCENES["mixed"]()) as b:
        ref = b.oracle(rays, samples, bounces)
        got = {p: b.query(rays, samples, bounces, p) for p in (0, 1)}
    lit = float((ref[:, :3] > 0).any(axis=1).mean())
    print(samples, bounces, "lit", lit)
    assert lit >= (0.9 if bounces > 1 else 0.25)                     # one bounce: only the sky and the emitters are lit
    for p, g in got.items():
        assert equal(g, ref), (samples, bounces, p, where_differs(g, ref, rays))


def test_batch_sizes_around_a_wave_and_a_workgroup(ctx):
    """n around the resident-grid kernel's refill threshold (16 free lanes), a wave and a workgroup, against the oracle."""
    rays = probes(np.random.default_rng(52), 257, BOX["mixed"])
    with Bound(ctx, SCENES["mixed"]()) as b:
        ref = b.oracle(rays, 2, 4)
        got = {(n, p): b.query(rays[:n], 2, 4, p, device=(n == 65)) for n in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257) for p in (0, 1)}
    assert (ref[:, :3] > 0).any(axis=1).mean() >= 0.9
    for (n, p), g in got.items():
        assert g.shape == (n, 4) and equal(g, ref[:n]), (n, p, where_differs(g, ref[:n], rays))


# ---- C. the resident-grid kernel beyond its grid ------------------------------------------------------------------------------------
def beyond_the_grid(ctx):
    """n = 2 * CUs * 2048 + 77.  A CU holds at most 2048 threads, so the resident grid has at most CUs * 2048 lanes whatever the
    occupancy query returns, and a lane's first draw covers at most that many queries: more than half of the batch is necessarily taken
    by lanes that have finished a query before — the refill path."""
    import torch
    return 2 * torch.cuda.get_device_properties(torch.device("cuda", ctx.device)).multi_processor_count * 2048 + 77


@pytest.fixture(scope="module")
def big(ctx):
    """The big rays-mode batch, its oracle answers (mode 0, every query) and its first-hit kinds: computed once, never changed."""
    n = beyond_the_grid(ctx)
    rng = np.random.default_rng(61)
    rays = probes(rng, n, BOX["mixed"], seeds=(0.0, 8.0))
    rays[:, 8:10] = rng.integers(0, 4096, (n, 2))
    with Bound(ctx, SCENES["mixed"]()) as b:
        ref = b.oracle(rays, 2, 4)
        kind = b.kinds(rays)
    lit = float((ref[:, :3] > 0).any(axis=1).mean())
    distinct = len(np.unique(ref[:, :3].view(np.uint32), axis=0))
    print("n", n, "lit", lit, "distinct RGB", distinct, "kinds", np.bincount(kind, minlength=4).tolist())
    assert lit >= 0.9 and distinct > n // 2                          # a query answered with another's result cannot pass
    for a in (rays, ref, kind):
        a.setflags(write=False)
    return rays, ref, kind


@pytest.mark.parametrize("persist", [1, 0])
def test_rays_beyond_the_grid(ctx, big, persist):
    """See beyond_the_grid: with radiance_persist = 1 more than half of these queries run on a refilled lane (s, k, avg re-initialised,
    the prefix popcount over a partial dead mask, neighbours mid-path); radiance_persist = 0 is the same batch one query per thread."""
    rays, ref, _ = big
    with Bound(ctx, SCENES["mixed"]()) as b:
        got = b.query(rays, 2, 4, persist)
    assert equal(got, ref), (persist, where_differs(got, ref, rays))


def test_rays_beyond_the_grid_sorted_by_first_hit(ctx, big):
    """The same batch sorted by first-hit kind: whole waves die at once on the sky and others not at all.  A query's answer does not
    depend on its place in the batch."""
    rays, ref, kind = big
    order = np.argsort(kind, kind="stable")
    assert len(np.unique(kind)) == 4
    with Bound(ctx, SCENES["mixed"]()) as b:
        got = {p: b.query(np.ascontiguousarray(rays[order]), 2, 4, p, device=(p == 1)) for p in (1, 0)}
    for p, g in got.items():
        back = np.empty_like(g)
        back[order] = g
        assert equal(back, ref), (p, where_differs(back, ref, rays))


@pytest.mark.parametrize("persist", [1, 0])
def test_pixels_beyond_the_grid_with_runs_of_refused_pixels(ctx, persist):
    """Pixels mode, device form, the 960 pixels of a 40 x 24 Result repeated to the same n (beyond_the_grid), with three runs of pixels
    outside the Result — 8,192 at the start, 8,192 across n / 2, the last 300 — so that whole waves draw nothing but refused pixels and
    must draw again.  Valid queries equal the oracle's literal render of their pixel (frame 0's uniforms), refused ones four zero
    words."""
    import torch
    n = beyond_the_grid(ctx)
    rays_per_pixel, bounces, seed, off = 2, 4, 0.4375, (0.3125, 0.71875)
    sc = copy.copy(SCENES["mixed"]())
    sc.num_rays, sc.num_bounces, sc.seed, sc.pixel_offset = rays_per_pixel, bounces, seed, off
    X, Y = np.meshgrid(np.arange(W, dtype=np.int32), np.arange(H, dtype=np.int32))
    xy = np.tile(np.stack([X.reshape(-1), Y.reshape(-1)], axis=1), (n // (W * H) + 1, 1))[:n].copy()
    refused = np.zeros(n, bool)
    refused[:8192] = refused[n // 2 - 4096:n // 2 + 4096] = refused[n - 300:] = True
    outside = np.array([(-1, 5), (W, 0), (0, H), (7, -1), (-2147483648, 3), (2147483647, 2147483647), (W + 216, H + 232), (3, 65536)], np.int32)
    xy[refused] = outside[np.arange(int(refused.sum())) % len(outside)]
    m = RayTraceMaster(ctx, sc)
    m.numRays, m.numBounces = rays_per_pixel, bounces
    ctx.set_option("radiance_persist", persist)
    try:
        got = m.ResamplePixels(torch.from_numpy(xy).to(torch.device("cuda", ctx.device))).cpu().numpy()      # frame 0: the scene's own offset and seed
    finally:
        ctx.set_option("radiance_persist", -1)
        m.OnDisable()
    orc = pyoracle.Oracle(sc)
    orc.set_frame(off, seed)
    frame = orc.render(mode=0, threads=THREADS)
    ref = frame[xy[~refused, 1], xy[~refused, 0]]
    assert (frame[..., :3] > 0).any(axis=2).mean() >= 0.9
    assert not got[refused].view(np.uint32).any()                    # four zero words, not (0, 0, 0, 1)
    assert equal(got[~refused], ref), (persist, where_differs(got[~refused], ref, xy[~refused].astype(F)))
