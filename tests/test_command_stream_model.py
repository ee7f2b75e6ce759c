"""CPU: the command-stream generator reaches the cases the GPU test exists for, and the sequential model is the documented frame loop.

These are conditions, not measurements: they keep tests/test_gpu_command_stream.py from passing by never getting to a written texture
bound as the sky, a readback over deferred frames or a scene edit inside a batch — and tests/test_gpu_command_stream_pipeline.py from
passing by never feeding an image operation what deferred frames wrote, never writing vertices on the device inside a batch, never
editing the scene behind an un-waited query, or by reprojecting, selecting and denoising images in which nothing happens — and
tests/test_gpu_command_stream_display.py from passing by never metering, blooming, tone-mapping or upsampling what deferred frames
wrote, never chaining an exposure state un-waited, never writing the bound Result texture or the next sky with a display call, never
regrowing the bloom pyramid, or by metering images in which nothing counts — and tests/test_gpu_command_stream_dynamic.py from
passing by never building a heap on the device between deferred frames, behind an upload, a morph or an un-waited query, never reading
back or overwriting a device-written heap, never morphing twice in a row, never blurring what deferred frames wrote, or by heaps,
weights and blurs that change nothing of what is compared — and tests/test_gpu_command_stream_solo.py from passing by never changing
the camera, the scene or the Result texture between two frames of what would be one batch of the single-mesh kernel, never following
a vertex write of each kind by a frame that nothing has looked at the vertices before, never motion-blurring what deferred frames
wrote, into the bound Result or into the next sky, or by motion blurs that change nothing."""
import numpy as np
import pytest

from oracle import pyoracle
from unityraytracer_amd import scenes

import command_stream as cs

SEEDS = range(24)                                                # the seed set of tests/test_gpu_command_stream.py


def test_programs_are_deterministic_per_seed():
    for seed in (0, 7, 23):
        assert cs.make_program(seed) == cs.make_program(seed)
    assert cs.make_program(1) != cs.make_program(2)
    for seed in SEEDS:
        p = cs.make_program(seed)
        assert 40 <= len(p) <= 42, (seed, len(p))               # (40 ops, then the ReadEnd of whatever is still in flight)
        tr = cs._Track()
        for op in p:                                             # every program keeps to the rules of the module's docstring
            assert op[0] in cs.KINDS and tr.allowed(op), (seed, op)
            tr.apply(op)
        assert tr.tickets == 0


def test_seed_set_reaches_the_interesting_cases():
    cov = [cs.coverage(cs.make_program(seed)) for seed in SEEDS]
    kinds = {k: sum(c["kinds"][k] for c in cov) for k in cs.KINDS}
    sky_after = {w: sum(w in c["sky_after"] for c in cov) for w in cs.WRITER_KINDS}
    reads = sum(c["read_while_deferred"] > 0 for c in cov)
    edits = sum(c["edit_between_frames"] > 0 for c in cov)
    print("op kinds over the seed set:", kinds)
    print("programs that bind a texture as the sky after ... wrote it, and trace:", sky_after)
    print("programs that read back over deferred frames:", reads, " that edit the scene inside a batch:", edits)
    assert all(n >= 10 for n in kinds.values()), kinds
    assert all(n >= 1 for n in sky_after.values()), sky_after
    assert reads >= 3 and edits >= 3


def oracle_frame(sc, sky, frame):
    s = cs.copy.copy(sc)
    s.sky = sky
    s.pixel_offset, s.seed = cs.frame_uniforms_of(sc, frame)
    return pyoracle.Oracle(s).render(mode=0, threads=8)


def test_model_of_hand_written_programs():
    sc = cs.make_scene()
    zeros = np.zeros((sc.height, sc.width, 4), np.float32)
    # one frame
    obs, tex = cs.run_model([("frame", None), ("get", "T0")])
    f0 = oracle_frame(sc, sc.sky, 0)
    assert f0.any() and len(obs) == 1 and obs[0][:2] == (1, "get") and cs.same(obs[0][2], f0)
    assert cs.same(tex["T0"], f0) and cs.same(tex["C"], pyoracle.accumulate(f0, zeros, 0.0)) and cs.same(tex["X0"], zeros)
    # frame + blend + present, twice, read back in a converted format
    obs, tex = cs.run_model([("frame", "X0"), ("frame", "X0"), ("read_begin", "X0", "RGBA16F"), ("get", "C"), ("read_end",)])
    f1 = oracle_frame(sc, sc.sky, 1)
    c = pyoracle.accumulate(f1, pyoracle.accumulate(f0, zeros, 0.0), 1.0)
    assert [o[:2] for o in obs] == [(3, "get"), (4, "read_end")]
    assert cs.same(obs[0][2], c) and cs.same(obs[1][2], c.astype(np.float16)) and cs.same(tex["X0"], c) and cs.same(tex["T0"], f1)
    # blit into the sky, then a frame: the frame samples the NEW sky
    obs, tex = cs.run_model([("setpixels", "S1", 1.5), ("blit", "S1", "S0"), ("frame", None), ("get", "T0")])
    flat = np.full_like(sc.sky, 1.5)
    want = oracle_frame(sc, flat, 0)
    assert cs.same(tex["S0"], flat) and cs.same(obs[0][2], want) and not cs.same(want, f0)


# ---- the pipeline profile ------------------------------------------------------------------------------------------------------------
F = np.float32
# sha256 of repr([make_program(seed) for seed in range(24)]), computed on the commit before the pipeline profile existed
FRAME_PROGRAMS_DIGEST = "770ff5c6ab1c8963024ba34dadfc434fbea4f3047bc31b8d365e4f72afb1fb99"
# ... and of repr([make_program(seed, profile="pipeline") for seed in range(24)]), computed on the commit before the display profile existed
PIPELINE_PROGRAMS_DIGEST = "ac84caddba71acdb56696727b1c59ba88ad9c0c1ea2d81fb6d7fe377db2341cb"
# ... and of repr([make_program(seed, profile="display") for seed in range(24)]), computed on the commit before the dynamic profile existed
DISPLAY_PROGRAMS_DIGEST = "63f148d9def3cd1d403ffa6a9b1770aa3091c52cc5a956935e9328b74ceb8c84"


def pipeline(ops, **kw):
    return cs.run_model(ops, profile="pipeline", **kw)


def test_the_frame_loop_programs_are_what_they_were():
    import hashlib
    programs = [cs.make_program(seed) for seed in SEEDS]
    assert hashlib.sha256(repr(programs).encode()).hexdigest() == FRAME_PROGRAMS_DIGEST
    assert programs == [cs.make_program(seed, profile="frames") for seed in SEEDS]
    assert not any(op[0] in cs.NEW_KINDS for p in programs for op in p)
    piped = [cs.make_program(seed, profile="pipeline") for seed in SEEDS]
    assert hashlib.sha256(repr(piped).encode()).hexdigest() == PIPELINE_PROGRAMS_DIGEST
    assert not any(op[0] in cs.DISPLAY_KINDS for p in piped for op in p)
    displayed = [cs.make_program(seed, profile="display") for seed in SEEDS]
    assert hashlib.sha256(repr(displayed).encode()).hexdigest() == DISPLAY_PROGRAMS_DIGEST
    for p in programs + piped + displayed:                       # no older program holds a dynamic kind, or a buffer only that profile has
        assert not any(op[0] in cs.DYNAMIC_KINDS or (op[0] == "get_buffer" and op[1] in cs.HEAP_BUFFERS) for op in p)


def pipeline_op_keeps_to_the_rules(seed, op, tr, names=cs.ALL_TEX + cs.PIPE_TEX, world="mixed"):
    """The refusals of the pipeline profile's calls, for an op about to run in the state `tr`."""
    lo, hi = cs.pipeline_world(world=world)["span"]
    nv = len(cs.pipeline_world(world=world)["rest_v"])
    k = op[0]
    outputs = [t for t, _ in cs.pipeline_writes_of(op, tr.result)] if k in cs.IMAGE_OPS else []
    assert tr.sky not in outputs, (seed, op, "an output is the bound sky")
    if k != "resample":                                          # (resample_below blends into what it reads: its H and N are two textures)
        assert not set(outputs) & set(cs.pipeline_reads_of(op, tr.result)), (seed, op, "an output is also an input")
    named = [a for a in op[1:] if isinstance(a, str) and a in names]
    if k in cs.IMAGE_OPS + ("blit",):
        assert len({cs.size_class(n) for n in named}) <= 1, (seed, op, "sizes differ")
    if k == "aov":
        assert op[2] in range(1, 16)
    if k == "skin":
        assert lo <= op[3] and op[4] >= 1 and op[3] + op[4] - 1 <= hi and 0 <= op[1] < len(cs.POSE_ANGLES), (seed, op)
    if k in ("set_device", "set_host", "bounds"):
        assert 0 <= op[1] and op[2] >= 1 and op[1] + op[2] <= nv, (seed, op)
    if k == "get_buffer":
        assert op[1] in cs.BUFFERS and 0 <= op[2] and op[3] >= 1 and op[2] + op[3] <= nv, (seed, op)
    if k != "get" and k != "denoise":
        assert "D" not in op[1:], (seed, op, "the denoised image feeds something")


def test_pipeline_programs_keep_to_the_rules():
    assert cs.make_program(3, profile="pipeline") == cs.make_program(3, profile="pipeline") != cs.make_program(4, profile="pipeline")
    for seed in SEEDS:
        p = cs.make_program(seed, profile="pipeline")
        assert 40 <= len(p) <= 60, (seed, len(p))
        tr = cs._PipeTrack()
        for op in p:
            assert op[0] in cs.PIPE_KINDS and tr.allowed(op), (seed, op)
            pipeline_op_keeps_to_the_rules(seed, op, tr)
            tr.apply(op)
        assert tr.tickets == 0


@pytest.fixture(scope="module")
def pipeline_models():
    """The model of every program of the seed set with its figures, made once: [(program, observations, final, stats)]."""
    out = []
    for seed in SEEDS:
        p, stats = cs.make_program(seed, profile="pipeline"), []
        obs, fin = pipeline(p, stats=stats)
        out.append((p, obs, fin, stats))
    return out


def test_pipeline_seed_set_reaches_the_interesting_cases(pipeline_models):
    cov = [cs.pipeline_coverage(p) for p, _, _, _ in pipeline_models]
    kinds = {k: sum(c["kinds"][k] for c in cov) for k in cs.PIPE_KINDS}
    cases = {key: sum(c[key] > 0 for c in cov) for key in ("input_deferred", "output_deferred", "vertex_write_in_batch", "async_then_change",
                                                          "mixed_readback")}
    print("op kinds over the pipeline seed set:", kinds)
    print("programs in which ... occurs:", cases)
    assert all(kinds[k] >= 10 for k in cs.NEW_KINDS), kinds
    assert all(n >= 3 for n in cases.values()), cases
    # non-vacuity, on the model's own output
    stats = [s for _, _, _, st in pipeline_models for s in st]
    rp = [f for _, k, f in stats if k == "reproject"]
    good_rp = sum(f["kept"] >= 0.25 and f["lost"] >= 0.02 for f in rp)
    sel = [f for _, k, f in stats if k in ("select", "resample")]
    good_sel = sum(1 <= f["selected"] <= f["of"] for f in sel)
    partial = sum(1 <= f["selected"] < f["of"] for f in sel)
    dn = [f for _, k, f in stats if k == "denoise"]
    good_dn = sum(f["changed"] >= 1 and f["identical"] >= 1 for f in dn)
    print(f"reprojections that keep >= 25 % and lose >= 2 % of the pixels: {good_rp} of {len(rp)};  selections of 1 .. all pixels: {good_sel} of "
          f"{len(sel)} ({partial} of them not all);  denoise ops that change a surface pixel and keep one: {good_dn} of {len(dn)}")
    assert 2 * good_rp >= len(rp) and 2 * good_sel >= len(sel) and 2 * good_dn >= len(dn)
    assert partial >= 10
    # every async answer is observed, and the final contents hold both sides of every buffer
    for p, obs, fin, _ in pipeline_models:
        assert sum(op[0].endswith("_async") for op in p) == sum(k.endswith("_async") for _, k, _ in obs)
        assert all(n in fin and n + ".dev" in fin for n in cs.BUFFERS)


CHANGED = {"meter": lambda op: op[:2] + (1 - op[2],) + op[3:],                   # the other state
           "tonemap": lambda op: op[:5] + (op[5] * 4.0,),                        # two stops more
           "bloom": lambda op: op[:5] + (op[5] ^ cs.BLOOM_ONLY,),                # with / without the source
           "upsample": lambda op: op[:4] + (op[4] ^ cs.SKY_FROM_ALBEDO,)}


DYNAMIC_CHANGED = {"morph": lambda op: ("morph", (op[1] + 1) % len(cs.MORPH_WEIGHTS)) + op[2:],        # another weight table
                   "dof": lambda op: op[:4] + ((op[4] + 1) % len(cs.DOF),),                              # another preset
                   "device_heap": lambda op: ("device_heap", ("move_mesh", 1, 1) if op[1] != ("move_mesh", 1, 1) else ("move_mesh", 1, 0)),
                   "rebuild_heap": lambda op: ("rebuild_heap", 1 - op[1]),                               # the other kind's heap
                   "master_dof": lambda op: ("master_dof", 0 if op[1] is None else None)}              # on / off


def test_the_comparison_notices_one_changed_op(pipeline_models, display_models, dynamic_models, solo_models):
    """first_difference is not vacuous: leaving out one op that writes (the first of its kind in the program) shows, for most kinds at
    the very observation or texture it feeds — and so does changing one argument of one display call (the last of its kind in the
    program: what it writes is least likely to be overwritten)."""
    changed = set()
    for p, obs, fin, _ in display_models[:8]:
        for kind, change in CHANGED.items():
            at = [i for i, op in enumerate(p) if op[0] == kind]
            if not at or kind in changed:
                continue
            q = p[:at[-1]] + [change(p[at[-1]])] + p[at[-1] + 1:]
            assert q != p and len(q) == len(p) and [op[0] for op in q] == [op[0] for op in p]
            if cs.first_difference(cs.run_model(q, profile="display"), (obs, fin)) is not None:
                changed.add(kind)
    print("display kinds of which one changed argument was noticed:", sorted(changed))
    assert changed == set(CHANGED), changed
    noticed = {}
    for p, obs, fin, _ in pipeline_models[:8]:
        for kind in ("aov_into", "reproject", "denoise", "resample", "skin", "set_device", "set_host", "snapshot", "normals"):
            at = [i for i, op in enumerate(p) if op[0] == kind]
            if not at or kind in noticed:
                continue
            q = [op for i, op in enumerate(p) if i != at[0]]
            if sum(op[0] == "read_begin" for op in q) != sum(op[0] == "read_end" for op in q):
                continue
            try:
                other = pipeline(q)
            except AssertionError:
                continue
            same_obs = len(other[0]) == len(obs) and all(cs.same(a[2], b[2]) for a, b in zip(other[0], obs))
            same_fin = all(cs.same(np.asarray(other[1][n], fin[n].dtype), fin[n]) for n in fin)
            if not (same_obs and same_fin):
                noticed[kind] = True
    print("kinds whose removal the comparison noticed:", sorted(noticed))
    assert len(noticed) >= 7, noticed
    changed = set()
    for p, obs, fin, _ in dynamic_models[:8]:
        for kind, change in DYNAMIC_CHANGED.items():
            at = [i for i, op in enumerate(p) if op[0] == kind]
            if not at or kind in changed:
                continue
            q = p[:at[-1]] + [change(p[at[-1]])] + p[at[-1] + 1:]
            assert q != p and len(q) == len(p) and [op[0] for op in q] == [op[0] for op in p]
            if cs.first_difference(cs.run_model(q, profile="dynamic"), (obs, fin)) is not None:
                changed.add(kind)
    print("dynamic kinds of which one changed argument was noticed:", sorted(changed))
    assert changed == set(DYNAMIC_CHANGED), changed
    # the solo profile: the first motion_blur left out, and every scene change left out, one at a time: each of them shows (the final
    # contents hold both sides of V and NB, so an edit shows even where no frame follows it)
    blurs = shown_blurs = tried = shown = 0
    by_kind = {}
    for p, obs, fin, _ in solo_models[:8]:
        at = [i for i, op in enumerate(p) if op[0] == "motion_blur"]
        if at:
            blurs += 1
            shown_blurs += cs.first_difference(cs.run_model(p[:at[0]] + p[at[0] + 1:], profile="solo"), (obs, fin)) is not None
        for i, op in enumerate(p):
            kind = op[1][0] if op[0] == "device_heap" else op[0]
            if kind in cs.DEVICE_EDITS + ("camera",):
                tried += 1
                differs = cs.first_difference(cs.run_model(p[:i] + p[i + 1:], profile="solo"), (obs, fin)) is not None
                shown += differs
                by_kind[kind] = by_kind.get(kind, 0) + differs
    print(f"solo: the first motion_blur left out shows in {shown_blurs} of {blurs} programs; a scene change left out shows for {shown} of {tried}: {by_kind}")
    assert blurs >= 3 and shown_blurs == blurs, (blurs, shown_blurs)
    assert shown == tried and all(by_kind.get(k, 0) >= 1 for k in cs.DEVICE_EDITS + ("camera",) if k != "move_spheres"), (shown, tried, by_kind)


def test_model_of_feature_buffers():
    import aov_ref
    sc = cs.make_scene()
    ref = aov_ref.render_aov_ref(sc)
    obs, tex = pipeline([("aov", "G", 15, False), ("aov", "P", 5, False), ("aov_into", "C"), ("get", "Gi")])
    for name, img in zip(cs.G_TEX, ref):
        assert cs.same(tex[name], img), name
    assert cs.same(tex["Ph"], ref[0]) and cs.same(tex["Pa"], ref[2]) and not tex["Pn"].any() and not tex["Pi"].any()      # the subset only
    assert cs.same(tex["C"], ref[2]) and cs.same(obs[0][2], ref[3])
    # ... and the probe itself against the oracle's Trace, the numpy material table and the triangle the id names
    hit, nrm, alb, ident = ref
    kind, obj, prim = nrm[..., 3].astype(np.int32), ident.view(np.int32)[..., 0], ident.view(np.int32)[..., 1]
    assert set(np.unique(kind).tolist()) == {0, 1, 2, 3}
    O, D = aov_ref.camera_rays(sc, sc.width, sc.height)
    orc = pyoracle.Oracle(sc)
    for y, x in [(y, x) for y in range(0, sc.height, 7) for x in range(0, sc.width, 5)]:
        r = orc.trace(O[y, x] if O.ndim == 3 else O, D[y, x])
        assert r["kind"] == kind[y, x] and cs.same(F(r["distance"]).reshape(1), hit[y, x, 3:]) and cs.same(r["position"], hit[y, x, :3])
        assert cs.same(r["normal"], nrm[y, x, :3])
    surf = kind != 0
    tab = aov_ref.material_albedo(sc)
    m = aov_ref.material_index(sc, kind, obj)
    assert cs.same(alb[surf], tab[m[surf]])
    assert (obj[kind == 0] == -1).all() and (obj[kind == 1] == -1).all() and (prim[kind != 3] == -1).all() and (ident[..., 2:][kind != 3] == 0).all()
    assert all(cs.same(alb[y, x, :3], orc.sky(D[y, x])) and alb[y, x, 3] == 0 for y, x in zip(*np.nonzero(~surf)))
    tri = kind == 3
    v, ix = np.asarray(sc.vertices, np.float64).reshape(-1, 3), np.asarray(sc.indices).reshape(-1)
    mo = sc.mesh_objects[obj[tri]]
    assert ((prim[tri] >= mo["indices_offset"]) & (prim[tri] < mo["indices_offset"] + mo["indices_count"]) & ((prim[tri] - mo["indices_offset"]) % 3 == 0)).all()
    M = np.asarray(mo["localToWorldMatrix"], np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
    u, w = ident[..., 2][tri].astype(np.float64), ident[..., 3][tri].astype(np.float64)
    a, b, c = (v[ix[prim[tri] + k]] for k in range(3))
    local = a * (1 - u - w)[:, None] + b * u[:, None] + c * w[:, None]
    world = np.einsum("nij,nj->ni", M[:, :3, :3], local) + M[:, :3, 3]
    assert np.abs(world - hit[tri][:, :3]).max() < 1e-4                       # the point (primitive, u, v) names is the hit position
    # the frame ray is another ray, under the uniforms of the frame counter
    _, jit = pipeline([("frame", None), ("aov", "G", 1, True)])
    s1 = cs.copy.copy(sc)
    (s1.pixel_offset, s1.seed) = cs.frame_uniforms_of(sc, 1)
    want = aov_ref.render_aov_ref(s1, frame=(*s1.pixel_offset, s1.seed))[0]
    assert cs.same(jit["Gh"], want) and not cs.same(want, ref[0])


def test_model_of_the_temporal_step():
    from denoise_ref import denoise_ref
    from reproject_deform_ref import matrices_of, reproject_deformed_ref
    from reproject_motion_ref import reproject_objects_ref
    from reproject_ref import reproject_ref
    from resample_ref import blend_samples_ref, select_pixels_ref
    from unityraytracer_amd import host_scene
    sc = cs.make_scene()
    head = [("frame", None), ("history", 0.0), ("frame", None), ("history", 0.0), ("aov", "P", 11, False)]
    for form, change in (("plain", [("camera", 1)]), ("objects", [("move_mesh", 1, 2), ("move_spheres", 0), ("camera", 2)]),
                         ("deformed", [("snapshot",), ("skin", 1, True, 0, 98), ("camera", 1)])):
        mid = head + change + [("aov", "G", 15, False)]
        _, t = pipeline(mid)
        now = sc
        for op in change:
            if op[0] != "snapshot":
                now = cs.edited_scene(now, op)
        args = [t[n] for n in ("H", "N", "Ph", "Pn", "Pi", "Gh", "Gn", "Gi")] + \
               [scenes.world_to_clip(cs.cameras(sc)[0], sc.camera_inverse_projection), now.camera_to_world, now.camera_inverse_projection]
        tables = dict(mesh_motion=host_scene.mesh_motion(sc.mesh_objects, now.mesh_objects), sphere_motion=host_scene.sphere_motion(sc.spheres, now.spheres))
        if form == "plain":
            want = reproject_ref(*args, max_history=8.0)
        elif form == "objects":
            want = reproject_objects_ref(*args, max_history=8.0, **tables)
        else:
            deform = (np.asarray(sc.vertices, F).reshape(-1, 3), sc.indices, matrices_of(sc.mesh_objects), np.array([1, 0, 0], np.int32))
            want = reproject_deformed_ref(*args, max_history=8.0, deform=deform, **tables)
            assert want["kept"].sum() > 10, "no pixel takes the per-vertex path"
        stats = []
        obs, fin = pipeline(mid + [("reproject", form, 0, 8.0, "H"), ("select", "RN", 1.0), ("blit", "R", "H"), ("blit", "RN", "N"),
                                   ("resample", 1.0, 2, 4.0), ("denoise", "H", 2, True), ("get", "D")], stats=stats)
        count = np.ascontiguousarray(want["count"], F)
        assert 0.25 < (count[..., 0] > 0).mean() < 0.98, form
        xy = select_pixels_ref(count, 1.0)
        assert [o[1] for o in obs] == ["select", "resample", "get"] and cs.same(obs[0][2], xy) and obs[1][2].tolist() == [len(xy)] and len(xy) > 50
        assert cs.same(fin["MV"], np.ascontiguousarray(want["motion"], F)) and cs.same(fin["R"], np.ascontiguousarray(want["color"], F)), form
        s = cs.copy.copy(now)
        s.pixel_offset, s.seed = cs.frame_uniforms_of(sc, 2)                    # two frames have been dispatched
        s.num_rays = 2
        img = pyoracle.Oracle(s).render(mode=0, threads=8)
        h, n = blend_samples_ref(xy, img[xy[:, 1], xy[:, 0]], np.ascontiguousarray(want["color"], F), count, 1.0, 4.0)
        assert cs.same(fin["H"], h) and cs.same(fin["N"], n), form
        d = denoise_ref(h, fin["Gh"], fin["Gn"], fin["Ga"], iterations=2)
        assert fin["D"].dtype == np.float64 and np.array_equal(fin["D"], d, equal_nan=True) and np.array_equal(obs[2][2], d, equal_nan=True)
        assert cs.same(d.astype(F), fin["D"]) and not cs.same((d * 1.001).astype(F), fin["D"])       # (the bound `same` holds a denoised image to)
        assert [k for _, k, _ in stats] == ["reproject", "select", "resample", "denoise"]


def test_model_of_queries_and_async_answers():
    sc = cs.make_scene()
    ops = [("frame", None), ("radiance_pixels", 3), ("ray_query_async", 9), ("radiance_async", 9), ("deform", 0.75), ("move_spheres", 1),
           ("frame", None), ("radiance_query", 9), ("ray_query", 9)]
    obs, _ = pipeline(ops)
    assert [(i, k) for i, k, _ in obs] == [(1, "radiance_pixels"), (2, "ray_query_async"), (3, "radiance_async"), (7, "radiance_query"), (8, "ray_query")]
    s1 = cs.copy.copy(sc)
    s1.pixel_offset, s1.seed = cs.frame_uniforms_of(sc, 1)
    xy = cs.query_xy(3, sc.width, sc.height)
    assert cs.same(obs[0][2], pyoracle.Oracle(s1).render(mode=0)[xy[:, 1], xy[:, 0]])        # what the next frame writes to those pixels
    o, d = cs.query_rays(9)
    rays = pyoracle.path_rays(o, d, cs.query_pixels(), 0.25)
    assert cs.same(obs[2][2], pyoracle.radiance(pyoracle.Oracle(s1), rays, 1, 2))               # the scene at the call ...
    s2 = cs.edited_scene(cs.edited_scene(sc, ops[4]), ops[5])
    s2.pixel_offset, s2.seed = cs.frame_uniforms_of(sc, 2)
    assert cs.same(obs[3][2], pyoracle.radiance(pyoracle.Oracle(s2), rays, 1, 2)) and not cs.same(obs[2][2], obs[3][2])     # ... not at the observation
    early, late = obs[1][2], obs[4][2]
    orc = pyoracle.Oracle(sc)
    for j in range(cs.N_QUERIES):
        r = orc.trace(o[j], d[j])
        assert cs.same(early[j, :7], np.concatenate([[F(r["distance"])], r["position"], r["normal"]]).astype(F)) and early[j, 7:8].view(np.int32)[0] == r["kind"]
    assert early.shape == (cs.N_QUERIES, 12) and late.shape == (cs.N_QUERIES, 8)
    assert not cs.same(early[:, :7], late[:, :7])
    assert (early[:, 8].view(np.int32)[early[:, 7].view(np.int32) == 3] >= 0).all() and (early[:, 8].view(np.int32)[early[:, 7].view(np.int32) < 2] == -1).all()


def test_model_of_the_vertex_buffers():
    import normals_ref
    import skin_ref
    sc, w = cs.make_scene(), cs.pipeline_world()
    lo, hi = w["span"]
    v0, n0 = np.asarray(sc.vertices, F).reshape(-1, 3), np.asarray(sc.normals, F).reshape(-1, 3)
    assert (lo, hi) == cs.blob_span(sc) and cs.same(w["rest_v"][lo: hi + 1], v0[lo: hi + 1]) and not w["rest_v"][hi + 1:].any()
    assert cs.same(normals_ref.apply(w["plan"], v0), n0[lo: hi + 1])           # the plan recomputes the scene's own normals of the blob
    ops = [("snapshot",), ("skin", 2, True, lo + 10, 40), ("get_buffer", "V", lo, 60), ("get_buffer", "NB", lo, 60), ("bounds", lo, 60),
           ("set_host", lo + 30, 30, 1.25), ("set_device", 100, 30, 0.75), ("normals",), ("get_buffer", "SNAP", 0, 144), ("frame", None), ("get", "T0")]
    obs, fin = pipeline(ops)
    sl = slice(lo + 10, lo + 50)
    pos, nrm = skin_ref.skin(v0[sl], n0[sl], w["bone_idx"][sl], w["bone_wgt"][sl], w["poses"][2])
    v1, n1 = v0.copy(), n0.copy()
    v1[sl], n1[sl] = pos, nrm
    assert not cs.same(v1, v0) and cs.same(obs[0][2], v1[lo: lo + 60]) and cs.same(obs[1][2], n1[lo: lo + 60])
    b = skin_ref.bounds(v1, lo, 60)
    assert cs.same(obs[2][2], np.concatenate([b[0], b[1], [F(60)]]).astype(F))
    v2 = v1.copy()
    for first, count, scale in ((lo + 30, 30, 1.25), (100, 30, 0.75)):
        part = v2[first: first + count]
        c = part.mean(axis=0, dtype=np.float64).astype(F)
        v2[first: first + count] = (c + (part - c) * F(scale)).astype(F)
    n2 = n1.copy()
    n2[lo: hi + 1] = normals_ref.apply(w["plan"], v2)
    assert cs.same(obs[3][2], v0) and cs.same(fin["SNAP"], v0) and cs.same(fin["V"], v2) and cs.same(fin["V.dev"], v2) and cs.same(fin["NB"], n2)
    s = cs.copy.copy(sc)
    s.vertices, s.normals = v2, n2
    s.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(sc.mesh_objects, v2, sc.indices))
    assert cs.same(obs[4][2], oracle_frame(s, sc.sky, 0)) and not cs.same(obs[4][2], oracle_frame(sc, sc.sky, 0))


def test_model_of_six_plain_frames():
    sc = cs.make_scene()
    obs, tex = cs.run_model([("frame", None)] * 6)
    c = np.zeros((sc.height, sc.width, 4), np.float32)
    for k in range(6):
        c = pyoracle.accumulate(oracle_frame(sc, sc.sky, k), c, float(k))
    assert obs == [] and cs.same(tex["C"], c)
    assert scenes.frame_uniforms(3, cs.FRAME_SEED) != scenes.frame_uniforms(4, cs.FRAME_SEED)     # (the frames really differ)


# ---- the display profile -------------------------------------------------------------------------------------------------------------
def display(ops, **kw):
    return cs.run_model(ops, profile="display", **kw)


@pytest.fixture(scope="module")
def display_models():
    """The model of every display program of the seed set with its figures, made once: [(program, observations, final, stats)]."""
    out = []
    for seed in SEEDS:
        p, stats = cs.make_program(seed, profile="display"), []
        obs, fin = display(p, stats=stats)
        out.append((p, obs, fin, stats))
    return out


def test_display_programs_keep_to_the_rules():
    """Deterministic per seed, and no op the library would refuse: besides the pipeline profile's rules, the refusals of urt_upsample,
    urt_auto_exposure, urt_tonemap and urt_bloom (csrc/image_ops.cpp) and of RayTraceMaster.ToneMap."""
    assert cs.make_program(3, profile="display") == cs.make_program(3, profile="display") != cs.make_program(4, profile="display")
    names = cs.DISPLAY_EXACT + ("D",)
    seen = {"levels": set(), "bloom_flags": set(), "sizes": set(), "in_place": set(), "operators": set(), "upsample_flags": set(),
            "rates": set(), "meter_sizes": set()}
    for seed in SEEDS:
        p = cs.make_program(seed, profile="display")
        assert 40 <= len(p) <= 60, (seed, len(p))
        tr = cs._DisplayTrack()
        for op in p:
            k = op[0]
            assert k in cs.DISP_KINDS and tr.allowed(op), (seed, op)
            pipeline_op_keeps_to_the_rules(seed, op, tr, names)
            if k == "aov_low":
                assert tr.sky not in ("Lh", "Lm", "Lc", "Li"), (seed, op, "a target is the bound sky")
            if k == "upsample":                                  # unknown flags; one size per grid; an output that is an input or the sky
                _, color, count, with_low_count, flags = op
                assert flags in range(4) and isinstance(with_low_count, bool), (seed, op)
                outputs = [t for t in (color, count) if t is not None]
                assert len(set(outputs)) == len(outputs) and all(cs.size_class(t) == 0 and t in cs.DISPLAY_FRAME_TEX for t in outputs), (seed, op)
                assert tr.sky not in outputs and not set(outputs) & set(cs.display_reads_of(op, tr.result)), (seed, op)
                assert color in ("U", "X0", "H", tr.result) and count in ("UN", "N", None), (seed, op)
                seen["upsample_flags"].add(flags)
            if k == "meter":                                     # the parameter checks; a count image of another size
                _, src, s, with_count, j = op
                q = dict(key=0.18, min_exposure=1.0 / 64.0, max_exposure=64.0, rate=1.0, low_permille=100, high_permille=950, **{})
                q.update(cs.METER[j])
                assert all(np.isfinite(q[n]) and q[n] > 0 for n in ("key", "min_exposure", "max_exposure")) and q["min_exposure"] <= q["max_exposure"]
                assert q["rate"] > 0 and 0 <= q["low_permille"] < q["high_permille"] <= 1000, (seed, op)
                assert src in cs.DISPLAY_EXACT and s in (0, 1) and (not with_count or cs.size_class(src) == cs.size_class("N")), (seed, op)
                seen["rates"].add(q["rate"])
                seen["meter_sizes"].add(cs.size_class(src))
            if k in ("tonemap", "bloom"):                        # sizes that differ; a destination that is the bound sky
                _, src, dst, s, a, b = op
                assert src in cs.DISPLAY_EXACT and dst in cs.DISPLAY_EXACT and cs.size_class(src) == cs.size_class(dst), (seed, op)
                assert dst != tr.sky and s in (None, 0, 1), (seed, op)
                seen["sizes"].add((k, cs.size_class(src)))
                if src == dst:
                    seen["in_place"].add(k)
                if k == "tonemap":                               # an unknown operator, an exposure that is not finite and > 0
                    assert a in cs.TONEMAP_OPS and np.isfinite(b) and b > 0, (seed, op)
                    seen["operators"].add(a)
                else:                                            # levels outside 1 .. 16, unknown flag bits
                    assert 1 <= a <= 16 and b in (0, cs.BLOOM_ONLY), (seed, op)
                    seen["levels"].add(a)
                    seen["bloom_flags"].add(b)
            if k in ("state_get", "state_reset"):
                assert op[1] in (0, 1), (seed, op)
            if k == "present_tm":                                # ToneMap: the accumulated image, another size; tonemap / bloom: the sky
                assert op[1] is None or (op[1] in cs.DISPLAY_FRAME_TEX and op[1] not in ("C", tr.sky)), (seed, op)
                assert op[2] in cs.TONEMAP_OPS, (seed, op)
            if k == "get" and op[1] == "TM":
                assert tr.tm_ready, (seed, op, "the master owns no texture yet")
            tr.apply(op)
        assert tr.tickets == 0
    print("seen over the display seed set:", seen)
    assert {1, 3, 16} <= seen["levels"] and seen["bloom_flags"] == {0, cs.BLOOM_ONLY} and seen["operators"] == set(cs.TONEMAP_OPS)
    assert seen["sizes"] == {(k, c) for k in ("tonemap", "bloom") for c in (0, 1, 2)} and seen["in_place"] == {"tonemap", "bloom"}
    assert seen["upsample_flags"] == {0, 1, 2, 3} and {1.0, 0.25} <= seen["rates"] and seen["meter_sizes"] == {0, 1, 2}
    assert {m["rate"] for m in cs.METER} >= {1.0, 0.25} and any("low_permille" in m for m in cs.METER)
    assert cs.low_size(64, 40) == (24, 16) and {cs.size_class(n) for n in cs.LOW_TEX} == {2} and cs.size_class("U") == cs.size_class("C") == 0


def test_display_seed_set_reaches_the_interesting_cases(display_models):
    cov = [cs.display_coverage(p) for p, _, _, _ in display_models]
    kinds = {k: sum(c["kinds"][k] for c in cov) for k in cs.DISP_KINDS}
    keys = ("input_deferred", "output_deferred", "state_chain", "in_place_then_frame", "writes_bound_result", "pyramid_regrow",
            "two_meterings_rate_below_1")
    cases = {key: sum(c[key] > 0 for c in cov) for key in keys}
    sky = {w: sum(c["written_then_sky_traced"][w] > 0 for c in cov) for w in cs.DISPLAY_WRITERS}
    print("op kinds over the display seed set:", kinds)
    print("programs in which ... occurs:", cases)
    print("programs in which a texture last written by ... is bound as the sky and traced:", sky)
    assert all(kinds[k] >= 10 for k in cs.DISPLAY_KINDS) and all(kinds[k] >= 1 for k in cs.PIPE_KINDS), kinds
    assert all(n >= 3 for n in cases.values()), cases
    assert all(n >= 3 for n in sky.values()), sky
    # non-vacuity, on the model's own output
    stats = [s for _, _, _, st in display_models for s in st]
    up = [f for _, k, f in stats if k == "upsample"]
    good_up = sum(2 * f["result"] >= f["of"] for f in up)
    mt = [f for _, k, f in stats if k == "meter"]
    counted, moving = sum(f["counted"] > 0 for f in mt), sum(f["counted"] > 0 and not f["settled"] for f in mt)
    print(f"upsample ops with a result in at least half of the pixels: {good_up} of {len(up)};  meterings that count a texel: {counted} of "
          f"{len(mt)}, that leave the exposure on its way to the target: {moving}")
    assert 2 * good_up >= len(up) and 2 * counted >= len(mt) and moving >= 10
    for p, obs, fin, _ in display_models:                        # every state is in the final contents, every state_get is observed
        assert all(fin[n].shape == (cs.STATE_WORDS,) and fin[n].dtype == np.uint32 for n in cs.STATES + ("MS",)) and "TM" in fin
        assert sum(op[0] == "state_get" for op in p) == sum(k == "state_get" for _, k, _ in obs)
        assert all(n in fin for n in cs.LOW_TEX + cs.UP_TEX)


def test_model_of_the_exposure_state():
    import tonemap_ref as tm
    sc = cs.make_scene()
    f0 = oracle_frame(sc, sc.sky, 0)
    c = pyoracle.accumulate(f0, np.zeros_like(f0), 0.0)
    # a fresh state snaps to its target whatever the rate
    obs, fin = display([("frame", None), ("meter", "C", 0, False, 1), ("state_get", 0)])
    hist, counted, skipped = tm.luminance_histogram_ref(c)
    L = tm.metered_luminance(hist)
    target = min(max(F(0.18) / L, F(1.0 / 64.0)), F(64.0))
    assert counted > 1000 and counted + skipped == c.shape[0] * c.shape[1] and F(1.0 / 64.0) < target < F(64.0)
    want = cs.state_words({"exposure": target, "target": target, "counted": counted, "skipped": skipped, "hist": hist})
    assert obs[0][:2] == (2, "state_get") and cs.same(obs[0][2], want) and cs.same(fin["E0"], want) and not fin["E1"].any() and not fin["MS"].any()
    # a second metering at rate 0.25 moves a quarter of the way, in the header's arithmetic: prev + (target - prev) * rate
    obs, fin = display([("frame", None), ("meter", "C", 1, False, 1), ("meter", "S0", 1, False, 1), ("state_get", 1)])
    hist2, counted2, skipped2 = tm.luminance_histogram_ref(sc.sky)
    target2 = min(max(F(0.18) / tm.metered_luminance(hist2), F(1.0 / 64.0)), F(64.0))
    moved = target + (target2 - target) * F(0.25)
    assert moved.dtype == F and target2 != target and moved not in (target, target2)
    want = cs.state_words({"exposure": moved, "target": target2, "counted": counted2, "skipped": skipped2, "hist": hist2})
    assert cs.same(obs[0][2], want) and cs.same(fin["E1"], want) and not fin["E0"].any()
    # ... with the count image: texels without a sample are left out; a reset state is fresh again
    obs, fin = display([("frame", None), ("meter", "C", 0, True, 0), ("state_get", 0), ("history", 0.0), ("meter", "C", 0, True, 0), ("state_get", 0),
                        ("state_reset", 0), ("state_get", 0)])
    assert obs[0][2][2] == 0 and obs[0][2][3] == c.shape[0] * c.shape[1] and obs[0][2][0] == 0      # N is all zero: nothing counted, no exposure
    assert cs.same(obs[1][2][:4], cs.state_words({"exposure": target, "target": target, "counted": counted, "skipped": skipped, "hist": hist})[:4])
    assert not obs[2][2].any() and not fin["E0"].any()


def test_model_of_the_masters_tone_map():
    """present_tm is the three explicit calls on the master's own state, at the master's settings."""
    by_master = [("frame", None), ("master_bloom", True), ("present_tm", "X0", "aces"), ("frame", None), ("present_tm", "X0", "aces"),
                 ("master_bloom", False), ("present_tm", None, "reinhard"), ("get", "TM")]
    explicit = [("frame", None), ("meter", "C", 0, False, 3), ("bloom", "C", "X0", 0, 3, 0), ("tonemap", "X0", "X0", 0, "aces", 1.0),
                ("frame", None), ("meter", "C", 0, False, 3), ("bloom", "C", "X0", 0, 3, 0), ("tonemap", "X0", "X0", 0, "aces", 1.0),
                ("meter", "C", 0, False, 3), ("tonemap", "C", "X1", 0, "reinhard", 1.0), ("get", "X1")]
    assert cs.METER[3] == cs.MASTER_EXPOSURE and cs.MASTER_BLOOM == {"levels": 3}
    (obs_a, a), (obs_b, b) = display(by_master), display(explicit)
    assert cs.same(a["X0"], b["X0"]) and cs.same(a["TM"], b["X1"]) and cs.same(obs_a[0][2], obs_b[0][2]) and cs.same(a["MS"], b["E0"])
    assert a["MS"][0] != a["MS"][1] and a["MS"][0] != 0          # (the third metering did not snap: the state's history is in it)
    assert not a["E0"].any() and not b["MS"].any() and not b["TM"].any() and a["X0"][..., :3].any() and a["TM"][..., :3].any()
    assert a["X0"][..., :3].max() <= 1.0 and not cs.same(a["X0"], a["TM"])
    # ... and the explicit calls are the restatements
    import bloom_ref
    import tonemap_ref as tm
    obs, fin = display([("frame", None), ("meter", "C", 0, False, 0), ("bloom", "C", "X0", 0, 3, cs.BLOOM_ONLY), ("tonemap", "C", "X1", 0, "linear", 2.0),
                        ("tonemap", "S0", "S0", None, "reinhard", 0.5)])
    e = fin["E0"][:1].view(F)[0]
    sc = cs.make_scene()
    assert cs.same(fin["X0"], bloom_ref.bloom_ref(fin["C"], exposure=e, levels=3, flags=bloom_ref.FLAG_ONLY)[0])
    assert cs.same(fin["X1"], tm.tonemap_ref(fin["C"], exposure=2.0, op=tm.LINEAR, state_exposure=e))
    assert cs.same(fin["S0"], tm.tonemap_ref(sc.sky, exposure=0.5, op=tm.REINHARD)) and fin["X0"][..., :3].any()


def test_model_of_upsampling_a_constant():
    """A constant low colour comes out as that constant wherever the call has a result (0.25: a power of two, so that the weighted sum
    is 0.25 times the sum of the weights exactly), the count as 1, everything else as 0."""
    import upsample_ref
    head = [("aov", "G", 15, False), ("aov_low", False)]
    obs, fin = display(head + [("setpixels", "Lc", 0.25), ("upsample", "U", "UN", False, cs.WIDE_FALLBACK), ("get", "U")])
    assert fin["Lc"].shape == (16, 24, 4) and fin["Lh"].any() and (fin["Lc"] == 0.25).all()
    ref = upsample_ref.upsample_ref(*[fin[n] for n in ("Lc", "Lh", "Lm", "Li", "Gh", "Gn", "Gi")], flags=cs.WIDE_FALLBACK)
    result = ref["result"]
    assert 0.5 < result.mean() < 1.0 and ref["sky"][result].any() and ref["surface"][result].any()
    assert (fin["U"][result] == 0.25).all() and not fin["U"][~result].any() and cs.same(obs[0][2], fin["U"])
    assert (fin["UN"][result][:, 0] == 1.0).all() and not fin["UN"][..., 1:].any() and not fin["UN"][~result].any()
    # the low count and the sky's albedo take part where the op says so
    _, with_n = display(head + [("setpixels", "Ln", 1.5), ("upsample", "H", "N", True, cs.WIDE_FALLBACK | cs.SKY_FROM_ALBEDO)])
    ref2 = upsample_ref.upsample_ref(*[with_n[n] for n in ("Lc", "Lh", "Lm", "Li", "Gh", "Gn", "Gi")], low_count=with_n["Ln"], albedo=with_n["Ga"],
                                     flags=cs.WIDE_FALLBACK | cs.SKY_FROM_ALBEDO)
    assert cs.same(with_n["H"], ref2["color"]) and cs.same(with_n["N"], ref2["count"])
    sky = ref2["sky"] & ref2["result"]
    assert sky.any() and cs.same(with_n["H"][sky][:, :3], with_n["Ga"][sky][:, :3]) and (np.abs(with_n["N"][ref2["result"]][:, 0] - 1.5) < 1e-6).all()


def test_display_coverage_counts_what_it_says():
    """The analysis the seed set is held to, on programs small enough to count by hand."""
    chain = [("meter", "C", 0, False, 1), ("bloom", "C", "X0", 0, 3, 0), ("tonemap", "X0", "X0", 0, "aces", 1.0)]
    c = cs.display_coverage([("frame", None)] + chain + [("bind_sky", "S1"), ("frame", None)])
    assert (c["input_deferred"], c["state_chain"], c["in_place_then_frame"], c["output_deferred"], c["writes_bound_result"]) == (1, 2, 1, 0, 0)
    c = cs.display_coverage([("frame", None), ("get", "C")] + chain + [("get", "X0"), ("frame", None)])      # everything was submitted and waited for
    assert (c["input_deferred"], c["state_chain"], c["in_place_then_frame"]) == (0, 0, 0)
    c = cs.display_coverage([("frame", None), chain[0], ("state_get", 0)] + chain[1:])                       # a wait between the metering and its readers
    assert (c["input_deferred"], c["state_chain"]) == (1, 0)
    c = cs.display_coverage([("frame", None), ("tonemap", "C", "T0", None, "aces", 1.0), ("frame", None)])
    assert (c["writes_bound_result"], c["output_deferred"], c["input_deferred"]) == (1, 1, 1)
    c = cs.display_coverage([("frame", None), ("bind_result",), ("tonemap", "C", "T0", None, "aces", 1.0), ("frame", None)])
    assert (c["writes_bound_result"], c["output_deferred"]) == (0, 1)                                         # (T0 is no longer the bound one)
    c = cs.display_coverage([("frame", None), ("tonemap", "C", "T0", None, "aces", 1.0)])
    assert (c["writes_bound_result"], c["output_deferred"]) == (0, 0)                                         # (no frame follows)
    blooms = [("bloom", "Lc", "Ln", None, 3, 0), ("bloom", "C", "X0", None, 3, 0), ("bloom", "C", "X0", None, 1, 0), ("bloom", "S0", "S1", None, 3, 0),
              ("bloom", "Lc", "Lc", None, 16, 0)]
    assert cs.display_coverage(blooms)["pyramid_regrow"] == 2 and cs.display_coverage(blooms[::-1])["pyramid_regrow"] == 1
    assert cs.pyramid_texels(24, 16, 3) == 12 * 8 + 6 * 4 + 3 * 2 < cs.pyramid_texels(64, 40, 3) < cs.pyramid_texels(128, 64, 3)
    sky = [("tonemap", "C", "X1", None, "aces", 1.0), ("upsample", "U", "UN", False, 1), ("bloom", "C", "X2", None, 3, 0)]
    c = cs.display_coverage(sky + [("bind_sky", "X1"), ("frame", "X0"), ("bind_sky", "UN"), ("frame", "X0"), ("frame", "X0")])
    assert c["written_then_sky_traced"] == {"upsample": 1, "tonemap": 1, "bloom": 0}
    c = cs.display_coverage(sky + [("setpixels", "X1", 0.25), ("bind_sky", "X1"), ("frame", "X0")])         # something else wrote it since
    assert c["written_then_sky_traced"] == {"upsample": 0, "tonemap": 0, "bloom": 0}
    c = cs.display_coverage([("bind_sky", "X2")] + sky + [("restart",), ("frame", "X0")])                     # bound before the write, too
    assert c["written_then_sky_traced"] == {"upsample": 0, "tonemap": 0, "bloom": 0}
    pairs = {(("C", 1), ("S0", 2)): 1, (("C", 1), ("X0", 1)): 0, (("C", 0), ("S0", 1)): 0, (("Lc", 3), ("C", 1)): 1}
    for ((a, ja), (b, jb)), n in pairs.items():                  # another size and both rates below 1
        assert cs.display_coverage([("meter", a, 0, False, ja), ("meter", b, 0, False, jb)])["two_meterings_rate_below_1"] == n, (a, ja, b, jb)
    assert cs.display_coverage([("meter", "C", 0, False, 1), ("meter", "S0", 1, False, 1)])["two_meterings_rate_below_1"] == 0   # two states


# ---- the dynamic profile -------------------------------------------------------------------------------------------------------------
def dynamic(ops, **kw):
    return cs.run_model(ops, profile="dynamic", **kw)


@pytest.fixture(scope="module")
def dynamic_models():
    """The model of every dynamic program of the seed set with its figures, made once: [(program, observations, final, stats)]."""
    out = []
    for seed in SEEDS:
        p, stats = cs.make_program(seed, profile="dynamic"), []
        obs, fin = dynamic(p, stats=stats)
        out.append((p, obs, fin, stats))
    return out


def test_the_dynamic_world_is_what_the_issue_asks_for():
    import morph_ref
    w = cs.dynamic_world()
    lo, hi = w["span"]
    _, _, (n_entries, max_valence, n_touched) = morph_ref.plan(w["deltas"], lo, hi - lo + 1)
    assert cs.N_TARGETS >= 3 and set(w["deltas"]["target"].tolist()) == set(range(cs.N_TARGETS))
    assert max_valence == cs.N_TARGETS > 1 and 0 < n_touched < hi - lo + 1 and n_entries == len(w["deltas"])      # touched by none, by all
    assert w["rest_v"] is cs.pipeline_world()["rest_v"]                           # the rest pose is in the buffers the skin ops use
    assert all(len(t) == cs.N_TARGETS for t in cs.MORPH_WEIGHTS) and not any(cs.MORPH_WEIGHTS[0])
    assert any(x < 0 for t in cs.MORPH_WEIGHTS for x in t)
    reaches = [p["max_radius"] for p in cs.DOF]
    assert any(r <= 4 for r in reaches) and any(4 < r <= 8 for r in reaches) and any(8 < r <= 16 for r in reaches)
    assert any(p.get("flags", 0) & cs.DOF_FLAG_COC for p in cs.DOF)
    sc = cs.make_scene()
    assert w["counts"] == {"LM": len(sc.mesh_objects), "LS": len(sc.spheres), "HM": len(sc.mesh_bvh), "HS": len(sc.sphere_bvh)}
    from unityraytracer_amd import _lib                            # the heap calls: counts that fit, at most URT_OBJECT_BVH_DEVICE_MAX leaves
    for leaves, heap in (("LM", "HM"), ("LS", "HS")):
        assert 0 < w["counts"][leaves] <= _lib.OBJECT_BVH_DEVICE_MAX and w["counts"][heap] == _lib.load().urt_host_object_bvh_length(w["counts"][leaves])
    assert "normals" not in cs.DEVICE_EDITS and set(cs.DEVICE_EDITS) == set(cs.SCENE_CHANGES) - {"normals"} | {"morph"}


def dynamic_op_keeps_to_the_rules(seed, op, tr, world="mixed"):
    """The refusals of urt_depth_of_field, urt_morph_vertices and the three heap calls (include/urt.h), for an op about to run in `tr`."""
    counts = cs.dynamic_world(world=world)["counts"]
    k = op[0]
    if k == "morph":                                             # URT_MORPH_NORMALIZE without dst_normals; the weights' count is n_targets
        _, j, with_normals, normalize = op
        assert 0 <= j < len(cs.MORPH_WEIGHTS) and len(cs.MORPH_WEIGHTS[j]) == cs.N_TARGETS, (seed, op)
        assert isinstance(with_normals, bool) and isinstance(normalize, bool) and (with_normals or not normalize), (seed, op)
    if k == "rebuild_heap":
        assert op[1] in (0, 1), (seed, op)
    if k == "dof":                                               # sizes that differ; dst == src, dst == hit, dst the bound sky; the parameters
        _, src, hit, dst, j = op
        assert hit in ("Gh", "Ph", "Lh") and src in cs.DISPLAY_EXACT and dst in cs.DISPLAY_EXACT, (seed, op)
        assert cs.size_class(src) == cs.size_class(hit) == cs.size_class(dst) in (0, 2), (seed, op, "sizes differ")
        assert dst not in (src, hit) and dst != tr.sky, (seed, op, "the destination is an input or the bound sky")
        q = dict(focus_distance=10.0, scale=8.0, max_radius=8.0, flags=0)
        q.update(cs.DOF[j])
        assert np.isfinite(q["focus_distance"]) and q["focus_distance"] > 0 and np.isfinite(q["scale"]) and q["scale"] >= 0, (seed, op)
        assert 0.5 <= q["max_radius"] <= 16.0 and q["flags"] in (0, cs.DOF_FLAG_COC), (seed, op)
    if k == "master_dof":
        assert op[1] is None or 0 <= op[1] < len(cs.DOF), (seed, op)
    if k == "present_tm" and tr.master_dof is not None:          # the blur's destination: not C (its source), not the bound sky
        assert op[1] is None or op[1] not in ("C", tr.sky), (seed, op)
    if k == "get_buffer" and op[1] in cs.HEAP_BUFFERS:
        assert 0 <= op[2] and op[3] >= 1 and op[2] + op[3] <= counts[op[1]], (seed, op)


def test_dynamic_programs_keep_to_the_rules():
    assert cs.make_program(3, profile="dynamic") == cs.make_program(3, profile="dynamic") != cs.make_program(4, profile="dynamic")
    names = cs.DISPLAY_EXACT + ("D",)
    seen = {"presets": set(), "dof_sizes": set(), "wrapped": set(), "morph_forms": set(), "rebuilt": set(), "buffers": set()}
    for seed in SEEDS:
        p = cs.make_program(seed, profile="dynamic")
        assert 40 <= len(p) <= 60, (seed, len(p))
        tr = cs._DynamicTrack()
        for op in p:
            k = op[0]
            assert k in cs.DYN_KINDS and tr.allowed(op), (seed, op)
            for inner in (op, op[1]) if k == "device_heap" else (op,):
                if inner[0] not in cs.DYNAMIC_KINDS and not (inner[0] == "get_buffer" and inner[1] in cs.HEAP_BUFFERS):
                    pipeline_op_keeps_to_the_rules(seed, inner, tr, names)
                dynamic_op_keeps_to_the_rules(seed, inner, tr)
            if k == "device_heap":                               # the leaves and the heap are never an input of their own build (two buffers each)
                assert op[1][0] in cs.DEVICE_EDITS and op[1][0] != "normals", (seed, op)
                seen["wrapped"].add(op[1][0])
            if k == "dof":
                seen["presets"].add(op[4])
                seen["dof_sizes"].add(cs.size_class(op[3]))
            if k == "morph":
                seen["morph_forms"].add(op[2:])
            if k == "rebuild_heap":
                seen["rebuilt"].add(op[1])
            if k == "get_buffer":
                seen["buffers"].add(op[1])
            tr.apply(op)
        assert tr.tickets == 0
    print("seen over the dynamic seed set:", seen)
    assert seen["presets"] == set(range(len(cs.DOF))) and seen["dof_sizes"] == {0, 2} and seen["wrapped"] == set(cs.DEVICE_EDITS)
    assert seen["morph_forms"] == {(False, False), (True, False), (True, True)} and seen["rebuilt"] == {0, 1}
    assert seen["buffers"] >= set(cs.HEAP_BUFFERS) | {"V"}


DYNAMIC_CASES = ("build_between_frames", "build_behind_upload", "build_behind_morph_or_skin", "host_write_of_device_heap", "get_device_heap",
                 "morph_after_morph", "async_across_build", "dof_input_deferred", "dof_into_result", "dof_regrow", "master_dof_then_frame",
                 "dof_sky_traced")


def test_dynamic_seed_set_reaches_the_interesting_cases(dynamic_models):
    cov = [cs.dynamic_coverage(p) for p, _, _, _ in dynamic_models]
    kinds = {k: sum(c["kinds"][k] for c in cov) for k in cs.DYN_KINDS}
    cases = {key: sum(c[key] > 0 for c in cov) for key in DYNAMIC_CASES}
    print("op kinds over the dynamic seed set:", kinds)
    print("programs in which ... occurs:", cases)
    assert all(kinds[k] >= 10 for k in cs.DYNAMIC_KINDS) and all(kinds[k] >= 1 for k in cs.DISP_KINDS), kinds
    assert all(n >= 3 for n in cases.values()), cases
    # non-vacuity, on the model's own output
    stats = [s for _, _, _, st in dynamic_models for s in st]
    dof = [f for _, k, f in stats if k == "dof"]
    changing, keeping = sum(f["changed"] >= 1 for f in dof), sum(f["identical"] >= 1 for f in dof)
    moving = sum(f["moved"] >= 1 for _, k, f in stats if k == "morph")
    print(f"dof ops that change a pixel of their source: {changing} of {len(dof)}, that leave one bit for bit: {keeping};  morph ops that move "
          f"a vertex: {moving}")
    assert 2 * changing >= len(dof) and keeping >= 5 and moving >= 10
    for p, obs, fin, _ in dynamic_models:                        # both sides of every buffer, the guide and every async answer
        assert all(n in fin and n + ".dev" in fin for n in cs.DYN_BUFFERS) and "DH" in fin
        assert all(fin[n].shape[1:] == (7,) and fin[n].dtype == np.uint32 for n in cs.HEAP_BUFFERS)
        assert sum(op[0].endswith("_async") for op in p) == sum(k.endswith("_async") for _, k, _ in obs)


def test_a_stale_heap_shows_in_what_is_compared(dynamic_models):
    """The heap matters: the model with ONE device build left stale (the edit applied, the old heap and leaves kept) differs in a later
    observation that is no readback of those buffers, or in a final texture."""
    images = lambda fin: [n for n in fin if n.split(".")[0] not in cs.DYN_BUFFERS]
    showing = tried = 0
    for p, obs, fin, _ in dynamic_models:
        for at in [i for i, op in enumerate(p) if op[0] == "device_heap"][:2]:
            if showing >= 12:
                break
            tried += 1
            obs2, fin2 = dynamic(p, stale_builds=(at,))
            seen = [(a, b) for (_, k, a), (_, _, b) in zip(obs, obs2) if not (k == "get_buffer" and a.dtype == np.uint32)]
            showing += (not all(cs.same(b, a) for a, b in seen)) or not all(cs.same(fin2[n], fin[n]) for n in images(fin))
    print(f"device builds whose stale heap shows in a later observation or a final texture: {showing} of {tried} tried")
    assert showing >= 10


def test_model_of_morphing():
    import morph_ref
    sc, w = cs.make_scene(), cs.dynamic_world()
    lo, hi = w["span"]
    v0, n0 = np.asarray(sc.vertices, F).reshape(-1, 3), np.asarray(sc.normals, F).reshape(-1, 3)
    # the zero table returns the rest pose to the bit, whatever was there
    obs, fin = dynamic([("deform", 0.75), ("get_buffer", "V", 0, 144), ("morph", 0, True, False), ("get_buffer", "V", 0, 144)])
    assert not cs.same(obs[0][2], v0) and cs.same(obs[1][2], v0) and cs.same(fin["V"], v0) and cs.same(fin["NB"], n0) and not fin["W"].any()
    # a table with a negative weight: the restatement, the weights in W, and the frame shows the pose
    obs, fin = dynamic([("morph", 2, True, True), ("frame", None), ("get", "T0")])
    pos, nrm = morph_ref.morph(w["rest_v"], w["rest_n"], w["deltas"], lo, hi - lo + 1, cs.MORPH_WEIGHTS[2], True)
    assert cs.same(fin["V"][lo: hi + 1], pos) and cs.same(fin["NB"][lo: hi + 1], nrm) and cs.same(fin["V"][hi + 1:], v0[hi + 1:])
    assert cs.same(fin["W"], np.array(cs.MORPH_WEIGHTS[2], F)) and (pos != v0[lo: hi + 1]).any() and (pos == v0[lo: hi + 1]).all(axis=1).any()
    assert not cs.same(obs[0][2], oracle_frame(sc, sc.sky, 0))
    # positions only: the normals stay
    _, fin = dynamic([("morph", 3, False, False)])
    assert cs.same(fin["NB"], n0) and not cs.same(fin["V"], v0)


def test_model_of_the_device_built_heaps():
    from unityraytracer_amd import host_scene
    sc = cs.make_scene()
    edit = ("move_mesh", 0, 1)
    moved = cs.edited_scene(sc, edit)
    leaves = host_scene.mesh_leaf_bounds(moved.mesh_objects, moved.vertices, moved.indices, literal=False)
    want = cs.heap_words(host_scene.build_object_bvh(leaves))
    outward = cs.heap_words(scenes.build_object_bvh(*scenes.mesh_bounds(moved.mesh_objects, moved.vertices, moved.indices)))
    n = cs.dynamic_world()["counts"]
    obs, fin = dynamic([("device_heap", edit), ("get_buffer", "HM", 0, n["HM"]), ("get_buffer", "LM", 1, 2), ("frame", None), ("get", "T0")])
    assert cs.same(obs[0][2], want) and cs.same(fin["HM"], want) and cs.same(fin["HM.dev"], want) and cs.same(obs[1][2], cs.heap_words(leaves)[1:3])
    assert want.shape == outward.shape and (want != outward).any(), "the outward-rounded heap is the same: the model's choice decides nothing"
    assert cs.same(fin["HS"], cs.heap_words(sc.sphere_bvh)) and not fin["LS"].any()          # the other kind is left alone
    s = cs.copy.copy(moved)
    s.mesh_bvh = host_scene.build_object_bvh(leaves)
    assert cs.same(obs[2][2], oracle_frame(s, sc.sky, 0)) and not cs.same(obs[2][2], oracle_frame(sc, sc.sky, 0))
    # the host's SetData of the heap after it (an unwrapped edit) brings the outward-rounded values back; a rebuild replaces them again
    _, fin = dynamic([("device_heap", edit), edit])
    assert cs.same(fin["HM"], outward) and cs.same(fin["LM"], cs.heap_words(leaves))
    _, fin = dynamic([edit, ("rebuild_heap", 0), ("rebuild_heap", 1)])
    assert cs.same(fin["HM"], want) and cs.same(fin["LS"], cs.heap_words(host_scene.sphere_leaf_bounds(sc.spheres)))
    assert cs.same(fin["HS"], cs.heap_words(host_scene.build_object_bvh(host_scene.sphere_leaf_bounds(sc.spheres))))
    # a stale build keeps the old heap under the edited lists (the probe of the test above)
    _, stale = dynamic([("device_heap", edit)], stale_builds=(0,))
    assert cs.same(stale["HM"], cs.heap_words(sc.mesh_bvh)) and not stale["LM"].any()
    zeros = np.zeros(2, scenes.BVHNODE_DT)
    zeros["vmin"][0, 0], zeros["vmax"][1, 2] = -0.0, -0.0
    assert not cs.heap_words(zeros).any()                        # a zero of either sign is one value


def test_model_of_depth_of_field():
    import dof_ref
    head = [("frame", None), ("frame", None), ("aov", "G", 15, False)]
    _, fin = dynamic(head + [("dof", "C", "Gh", "X0", cs.DOF_IN_FOCUS), ("dof", "C", "Gh", "X1", 4), ("aov_low", False), ("dof", "Lc", "Lh", "Ln", 1)])
    near = cs.dof_foreground(fin["Gh"])
    assert near.sum() > 100 and (~near).sum() > 100
    assert cs.same(fin["X0"][near], fin["C"][near]), "the in-focus preset does not leave the foreground's bits"
    assert (fin["X0"][~near][:, :3] != fin["C"][~near][:, :3]).any() and cs.same(fin["X0"][..., 3], fin["C"][..., 3])
    assert cs.same(fin["X0"], dof_ref.dof_ref(fin["C"], fin["Gh"], **cs.DOF[cs.DOF_IN_FOCUS]))
    a = dof_ref.coc_ref(fin["C"], fin["Gh"], **{k: v for k, v in cs.DOF[4].items() if k != "flags"})[0]
    assert cs.same(fin["X1"][..., 0], a) and cs.same(fin["X1"][..., 3], fin["C"][..., 3]) and a.max() == 8.0 and a[a > 0].min() == 0.5
    assert fin["Ln"].shape == (16, 24, 4) and cs.same(fin["Ln"], dof_ref.dof_ref(fin["Lc"], fin["Lh"], **cs.DOF[1])) and not cs.same(fin["Ln"], fin["Lc"])


def test_model_of_the_masters_tone_map_with_depth_of_field():
    """present_tm with depth of field on is the four explicit calls behind the guide through the sample centres, and leaves the camera
    as it was: the frame after it is the frame it would have been."""
    import aov_ref
    import dof_ref
    sc = cs.make_scene()
    j = 1
    by_master = [("frame", None), ("master_dof", j), ("master_bloom", True), ("present_tm", "X0", "aces"), ("frame", None), ("present_tm", None, "reinhard"),
                 ("master_dof", None), ("master_bloom", False), ("present_tm", "X1", "aces"), ("get", "TM")]
    (obs, a) = dynamic(by_master)
    s = cs.copy.copy(sc)
    p = np.array(sc.camera_inverse_projection, F).reshape(16).copy()
    p[12:16] += p[0:4] * F(1.0 / sc.width) + p[4:8] * F(1.0 / sc.height)
    s.camera_inverse_projection = p
    guide = aov_ref.render_aov_ref(s)[0]
    assert cs.same(a["DH"], guide) and not cs.same(guide, aov_ref.render_aov_ref(sc)[0])
    # the explicit calls: the guide set by hand into Ph (nothing else writes it), the master's state as E0
    f0 = oracle_frame(sc, sc.sky, 0)
    c0 = pyoracle.accumulate(f0, np.zeros_like(f0), 0.0)
    import bloom_ref
    import tonemap_ref as tm
    state = tm.auto_exposure_ref(c0, None, cs.fresh_state(), **cs.MASTER_EXPOSURE)
    blurred = dof_ref.dof_ref(c0, guide, **cs.DOF[j])
    bloomed = bloom_ref.bloom_ref(blurred, exposure=state["exposure"], **cs.MASTER_BLOOM)[0]
    first = tm.tonemap_ref(bloomed, exposure=1.0, op=tm.ACES, state_exposure=state["exposure"])
    assert not cs.same(blurred, c0) and cs.same(a["X0"], first)
    c1 = pyoracle.accumulate(oracle_frame(sc, sc.sky, 1), c0, 1.0)
    assert cs.same(a["C"], c1), "ToneMap changed the accumulated image or the frame behind it"
    state = tm.auto_exposure_ref(c1, None, state, **cs.MASTER_EXPOSURE)
    blurred = dof_ref.dof_ref(c1, guide, **cs.DOF[j])
    bloomed = bloom_ref.bloom_ref(blurred, exposure=state["exposure"], **cs.MASTER_BLOOM)[0]
    assert cs.same(obs[0][2], tm.tonemap_ref(bloomed, exposure=1.0, op=tm.REINHARD, state_exposure=state["exposure"])) and cs.same(a["TM"], obs[0][2])
    state = tm.auto_exposure_ref(c1, None, state, **cs.MASTER_EXPOSURE)
    assert cs.same(a["X1"], tm.tonemap_ref(c1, exposure=1.0, op=tm.ACES, state_exposure=state["exposure"])) and cs.same(a["MS"], cs.state_words(state))
    # ... and the display profile's model of the same ops without the two dynamic ones is the model with depth of field off
    plain = [op for op in by_master if op[0] != "master_dof"]
    assert cs.same(display(plain)[1]["X1"], dynamic(plain)[1]["X1"]) and not cs.same(dynamic(plain)[1]["X0"], a["X0"])


def test_dynamic_coverage_counts_what_it_says():
    """The analysis the seed set is held to, on programs small enough to count by hand."""
    build = ("device_heap", ("move_mesh", 0, 1))
    c = cs.dynamic_coverage([("frame", None), build, ("frame", None), ("get", "C")])
    assert (c["build_between_frames"], c["build_behind_upload"], c["async_across_build"], c["kinds"]["device_heap"], c["kinds"]["move_mesh"]) == (1, 0, 0, 1, 0)
    c = cs.dynamic_coverage([("frame", None), ("get", "C"), build, ("frame", None)])                          # nothing is deferred in front of it
    assert c["build_between_frames"] == 0
    c = cs.dynamic_coverage([("frame", None), build, ("get_buffer", "HM", 0, 7), ("get_buffer", "HM", 0, 7), ("frame", None)])
    assert (c["build_between_frames"], c["get_device_heap"]) == (0, 1)                                          # (the first readback took it)
    c = cs.dynamic_coverage([build, ("frame", None), ("get_buffer", "HM", 0, 7), ("move_mesh", 0, 2)])       # the preparation took it
    assert (c["get_device_heap"], c["host_write_of_device_heap"]) == (0, 0)
    c = cs.dynamic_coverage([build, ("move_spheres", 1), ("move_mesh", 0, 2), ("move_mesh", 0, 0)])
    assert c["host_write_of_device_heap"] == 1                                                                  # (the other kind's heap is not it)
    c = cs.dynamic_coverage([("set_host", 0, 8, 0.9), ("rebuild_heap", 1), ("rebuild_heap", 0), ("skin", 0, True, 0, 98), ("rebuild_heap", 0),
                             ("device_heap", ("deform", 0.9)), ("frame", None), ("rebuild_heap", 0)])
    assert (c["build_behind_upload"], c["build_behind_morph_or_skin"]) == (2, 1)
    c = cs.dynamic_coverage([("ray_query_async", 1), build, ("get", "C"), build, ("radiance_async", 1), ("frame", None), ("rebuild_heap", 0)])
    assert c["async_across_build"] == 2
    c = cs.dynamic_coverage([("morph", 1, True, False), ("morph", 1, False, False), ("morph", 2, True, False), ("frame", None), ("morph", 0, True, False)])
    assert c["morph_after_morph"] == 1
    g = ("aov", "G", 15, False)
    c = cs.dynamic_coverage([g, ("frame", None), ("dof", "C", "Gh", "T0", 0), ("frame", None), ("dof", "C", "Gh", "T0", 0)])
    assert (c["dof_input_deferred"], c["dof_into_result"]) == (2, 1)                                           # (no frame follows the second)
    c = cs.dynamic_coverage([("frame", None), g, ("dof", "X0", "Gh", "X1", 0)])
    assert c["dof_input_deferred"] == 0
    low, full = ("dof", "Lc", "Lh", "Ln", 0), ("dof", "C", "Gh", "X0", 0)
    assert cs.dynamic_coverage([full, low, low, full, full, low])["dof_regrow"] == 1
    c = cs.dynamic_coverage([full, ("bind_sky", "X0"), ("frame", "X1"), ("dof", "C", "Gh", "X2", 0), ("setpixels", "X2", 0.25), ("bind_sky", "X2"), ("frame", "X1")])
    assert c["dof_sky_traced"] == 1
    tm = ("present_tm", None, "aces")
    c = cs.dynamic_coverage([("frame", None), ("master_dof", 1), tm, ("bind_sky", "S1"), ("frame", None), tm, ("get", "TM"), ("master_dof", None), tm, ("frame", None)])
    assert c["master_dof_then_frame"] == 1


# ---- the solo profile ----------------------------------------------------------------------------------------------------------------
def solo(ops, **kw):
    return cs.run_model(ops, profile="solo", **kw)


@pytest.fixture(scope="module")
def solo_models():
    """The model of every solo program of the seed set with its figures, made once: [(program, observations, final, stats)]."""
    out = []
    for seed in SEEDS:
        p, stats = cs.make_program(seed, profile="solo"), []
        obs, fin = solo(p, stats=stats)
        out.append((p, obs, fin, stats))
    return out


def test_the_solo_world_is_one_mesh_and_no_sphere():
    from unityraytracer_amd.unity_api import debug_build_blas
    sc, mixed, w = cs.make_scene(world="solo"), cs.make_scene(), cs.dynamic_world(world="solo")
    assert len(sc.mesh_objects) == 1 and len(sc.spheres) == 0 and len(sc.sphere_bvh) == 0 and (sc.num_rays, sc.num_bounces) == (1, 2)
    for field in ("localToWorldMatrix", "albedo", "specular", "emission", "smoothness"):
        if field in sc.mesh_objects.dtype.names:
            assert np.array_equal(sc.mesh_objects[field][0], mixed.mesh_objects[field][0]), field
    assert np.array_equal(sc.sky, mixed.sky)
    nv = len(np.asarray(sc.vertices).reshape(-1, 3))
    assert w["span"] == cs.blob_span(sc) == (0, nv - 1) and len(w["rest_v"]) == nv            # the span is the whole vertex list
    assert w["counts"] == {"LM": 1, "LS": 0, "HM": len(sc.mesh_bvh), "HS": 0}
    assert debug_build_blas(sc.mesh_objects, sc.vertices, sc.indices)[4] > 8                    # deeper than the stack minimum
    assert cs.dynamic_world() is not w and len(cs.dynamic_world()["rest_v"]) != nv              # the caches are keyed by the world
    assert len(cs.MBLUR) == 4 and cs.MBLUR[0] == {} and cs.MBLUR[1] == dict(shutter=1.0, max_radius=4.0) and \
        cs.MBLUR[2] == dict(shutter=0.25, max_radius=0.5) and cs.MBLUR[3] == dict(flags=1)
    assert "move_spheres" not in cs.SOLO_KINDS and "motion_blur" in cs.SOLO_IMAGE_OPS and "motion_blur" in cs.SOLO_WRITERS


def solo_op_keeps_to_the_rules(seed, op, tr):
    """What the solo world has no meaning for, and the refusals of urt_motion_blur (include/urt.h), for an op about to run in `tr`."""
    k = op[0]
    assert k != "move_spheres" and "HS" not in op[1:] and "LS" not in op[1:], (seed, op, "an op of the spheres")
    if k == "move_mesh":
        assert op[1] == 0, (seed, op)
    if k == "rebuild_heap":
        assert op[1] == 0, (seed, op)
    if k == "motion_blur":                                       # sizes that differ; dst an input or the bound sky; the parameters
        _, src, hit, dst, j = op
        assert hit in ("Gh", "Ph") and src in cs.DISPLAY_FRAME_TEX and dst in cs.DISPLAY_FRAME_TEX, (seed, op)
        assert cs.size_class(src) == cs.size_class(dst) == cs.size_class(hit) == cs.size_class("MV") == 0, (seed, op, "sizes differ")
        assert dst not in (src, "MV", hit) and dst != tr.sky, (seed, op, "the destination is an input or the bound sky")
        assert tr.mv_ready and (tr.g_ready if hit == "Gh" else tr.p_ready), (seed, op, "nothing has written the motion or the hit image")
        q = dict(shutter=0.5, max_radius=16.0, flags=0)
        q.update(cs.MBLUR[j])
        assert 0.0 <= q["shutter"] <= 1.0 and 0.5 <= q["max_radius"] <= 16.0 and q["flags"] in (0, cs.MBLUR_FLAG_VELOCITY), (seed, op)


def test_solo_programs_keep_to_the_rules():
    assert cs.make_program(3, profile="solo") == cs.make_program(3, profile="solo") != cs.make_program(4, profile="solo")
    names = cs.DISPLAY_EXACT + ("D",)
    presets, wrapped = set(), set()
    for seed in SEEDS:
        p = cs.make_program(seed, profile="solo")
        assert 40 <= len(p) <= 60, (seed, len(p))
        assert any(op[0] == "frame" for op in p), seed
        tr = cs._SoloTrack()
        for op in p:
            k = op[0]
            assert k in cs.SOLO_KINDS and tr.allowed(op), (seed, op)
            for inner in (op, op[1]) if k == "device_heap" else (op,):
                if inner[0] not in cs.DYNAMIC_KINDS + ("motion_blur",) and not (inner[0] == "get_buffer" and inner[1] in cs.HEAP_BUFFERS):
                    pipeline_op_keeps_to_the_rules(seed, inner, tr, names, world="solo")
                dynamic_op_keeps_to_the_rules(seed, inner, tr, world="solo")
                solo_op_keeps_to_the_rules(seed, inner, tr)
            if k == "device_heap":
                wrapped.add(op[1][0])
            if k == "motion_blur":
                presets.add(op[4])
            tr.apply(op)
        assert tr.tickets == 0
    print("seen over the solo seed set: presets", presets, "wrapped", wrapped)
    assert presets == set(range(len(cs.MBLUR))) and wrapped == set(cs.DEVICE_EDITS) - {"move_spheres"}


def test_solo_seed_set_reaches_the_interesting_cases(solo_models):
    cov = [cs.solo_coverage(p) for p, _, _, _ in solo_models]
    kinds = {k: sum(c["kinds"][k] for c in cov) for k in cs.SOLO_KINDS}
    cases = {key: sum(c[key] > 0 for c in cov) for key in cs.SOLO_CASES}
    print("op kinds over the solo seed set:", kinds)
    print("programs in which ... occurs:", cases)
    few = {k: kinds[k] for k in cs.DYNAMIC_KINDS + ("camera", "bind_result", "skin", "set_device", "set_host") if kinds[k] < 5}
    assert kinds["motion_blur"] >= 10 and not few, few
    assert all(n >= 3 for n in cases.values()), cases
    stats = [s for _, _, _, st in solo_models for s in st]      # non-vacuity, on the model's own output
    blur = [f for _, k, f in stats if k == "motion_blur"]
    changing, keeping = sum(f["changed"] >= 1 for f in blur), sum(f["identical"] >= 1 for f in blur)
    print(f"motion_blur ops that change a pixel of their source: {changing} of {len(blur)}, that leave one bit for bit: {keeping}")
    assert 2 * changing >= len(blur) and keeping >= 5
    for p, obs, fin, _ in solo_models:                           # both sides of every buffer that exists, and every async answer
        assert all(n in fin and n + ".dev" in fin for n in cs.DYN_BUFFERS if n not in ("LS", "HS")) and "LS" not in fin and "HS" not in fin
        assert sum(op[0].endswith("_async") for op in p) == sum(k.endswith("_async") for _, k, _ in obs)


def test_solo_coverage_counts_what_it_says():
    """The analysis the seed set is held to, on programs small enough to count by hand."""
    f, cam = ("frame", None), ("camera", 1)
    c = cs.solo_coverage([f, cam, f, ("get", "C"), cam, f, f, ("deform", 0.9), f])
    assert (c["camera_between_frames"], c["edit_between_frames"], c["kinds"]["camera"]) == (1, 1, 2)     # (nothing is open in front of the second camera)
    c = cs.solo_coverage([f, ("deform", 0.9), cam, f, f, cam, ("deform", 0.9), f, f, ("deform", 0.9), ("get", "C"), f])
    assert (c["edit_between_frames"], c["camera_between_frames"]) == (0, 2)                                 # a camera op or an observer between the frames
    c = cs.solo_coverage([f, ("bind_result",), f, ("bind_result",), cam, f, ("flush",), ("bind_result",), f])
    assert c["bind_result_between_frames"] == 1
    pre = [f, ("history", 0.0), ("aov", "P", 11, False), ("aov", "G", 15, False), ("reproject", "plain", 1, 8.0, "C")]
    blur = ("motion_blur", "C", "Gh", "X0", 0)
    c = cs.solo_coverage(pre + [blur, f, blur, f, ("get", "C"), ("motion_blur", "X1", "Ph", "X0", 0)])
    assert (c["blur_input_deferred"], c["two_presets"], c["blur_into_result_or_sky"]) == (1, 0, 0)         # (the first: the reproject has submitted)
    c = cs.solo_coverage(pre + [("motion_blur", "C", "Gh", "T0", 1), f, ("motion_blur", "C", "Gh", "T0", 2), blur, ("bind_sky", "X0"), f,
                                ("motion_blur", "C", "Gh", "X1", 2), ("setpixels", "X1", 0.25), ("bind_sky", "X1"), f])
    assert (c["blur_into_result_or_sky"], c["two_presets"], c["blur_input_deferred"]) == (3, 1, 2)         # (T0 twice, X0 as the sky; X1 is overwritten)
    c = cs.solo_coverage([("skin", 0, True, 0, 98), f, ("morph", 1, True, False), ("get_buffer", "V", 0, 8), f, ("device_heap", ("set_device", 0, 8, 0.9)),
                          ("bind_sky", "S1"), f, ("set_host", 0, 8, 0.9), ("aov", "G", 15, False), f, ("set_host", 0, 8, 0.9), ("rebuild_heap", 0), f])
    assert [c["write_then_frame_" + k] for k in cs.SOLO_VERTEX_WRITES] == [1, 0, 1, 0]


def test_model_of_motion_blur():
    import motion_blur_ref
    head = [("frame", None), ("frame", None), ("history", 0.0), ("aov", "P", 11, False)]
    tail = [("aov", "G", 15, False), ("reproject", "plain", 0, 8.0, "C")]
    blurs = [("motion_blur", "C", "Gh", "X0", 0), ("motion_blur", "C", "Gh", "X1", 1), ("motion_blur", "C", "Gh", "X2", 3), ("motion_blur", "C", "Ph", "U", 2)]
    _, moved = solo(head + [("camera", 1)] + tail + blurs)
    for dst, hit, j in (("X0", "Gh", 0), ("X1", "Gh", 1), ("X2", "Gh", 3), ("U", "Ph", 2)):          # the op is the restatement on the textures
        assert cs.same(moved[dst], motion_blur_ref.motion_blur_ref(moved["C"], moved["MV"], moved[hit], **cs.MBLUR[j])), (dst, j)
    assert (moved["MV"][..., 2] > 0).any() and (moved["Gh"][..., 3] > 0).any() and np.isinf(moved["Gh"][..., 3]).any()
    assert (moved["X0"][..., :3] != moved["C"][..., :3]).any(), "a moved camera leaves the image as it was"
    assert cs.same(moved["X0"][..., 3], moved["C"][..., 3]) and not cs.same(moved["X0"], moved["X1"])
    v = motion_blur_ref.velocity_ref(moved["C"], moved["MV"], moved["Gh"], max_radius=16.0)
    assert cs.same(moved["X2"][..., 2], np.where(v[4], v[2], np.float32(0.0)).astype(np.float32))      # the velocity preset writes the pixel's own length
    # a still motion image (no camera or scene change in front of the reproject): every tile is still, every pixel passes through
    _, still = solo(head + tail + blurs[:2])
    assert np.abs(still["MV"][..., :2]).max() < 1e-3 and (still["MV"][..., 2] > 0).any()      # (rounding only: far below the half pixel of a still tile)
    assert cs.same(still["X0"], still["C"]) and cs.same(still["X1"], still["C"]) and still["C"][..., :3].any()
