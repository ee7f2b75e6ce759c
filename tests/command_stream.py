"""Random command streams, a sequential model of them, and a runner (no GPU needed to import; tests/test_command_stream_model.py,
tests/test_gpu_command_stream.py).

The library defers: dispatches wait in a batch, the blends / presents behind them are queued, small launches alternate between two
trace streams behind a narrow dependency (csrc/frame_batch.cpp flush_pending).  The contract is PROGRAM ORDER: every call behaves as
if it ran alone, at once, on one stream.  A program here is a list of plain op tuples over a small fixed world; `run_model` executes it
sequentially with numpy arrays as textures and the oracle as the trace kernel, `run_gpu` executes it through the Python API.

The world: scenes.mixed_test_scene(width, height) with `bounces` bounces and one ray, ONE RayTraceMaster, and these textures:
    T0, T1      the two Result textures (the master's _target is one of them; "bind_result" swaps — to the library that is what a
                second camera's _target is: another Result texture under the same bindings)
    C           the master's _converged
    X0, X1, X2  frame-sized extras (present destinations, blit partners)
    H, N        a history / count pair for blit_add_history
    S0, S1      the scene's own sky and another texture of its size
Ops (first element = kind):
    ("frame", dest | None)             OnRenderImage(dest): dispatch, additive blend into C, optional present
    ("dispatch", "T0" | "T1")          bare dispatch into that Result texture, no blend (advances the frame sequence)
    ("blit", src, dst)                 Graphics.Blit between two textures of one size
    ("history", max_history)           ctx.blit_add_history(_target, H, N, max_history)
    ("setpixels", tex, value)          SetPixels(constant)
    ("restart",)                       _currentSample = 0
    ("bind_sky", tex | None)           _SkyboxTexture = tex (reaches the library at once)
    ("bind_result",)                   the master's _target becomes the other Result texture
    ("move_mesh", k, j)                SetData of _MeshObjects with object k at MOVES[j], and of the rebuilt heap
    ("deform", scale)                  ranged SetData of the blob's vertices scaled about their centre, and of the rebuilt heap
    ("move_spheres", j)                SetData of _Spheres shifted by SHIFTS[j], and of the rebuilt heap
    ("camera", j)                      _CameraToWorld = CAMERAS[j]
    ("flush",)                         ctx.flush()
    ("ptr", tex)                       device_ptr() (pointer hand-out: the image is never renamed again)
    ("get", tex)                       observer: GetPixels
    ("read_begin", tex, fmt)           observer: ReadBegin (at most two tickets in flight); observed at the matching
    ("read_end",)                      ... ReadEnd of the oldest ticket
    ("ray_query", seed)                observer: 64 closest-hit queries
    ("radiance_query", seed)           observer: 64 radiance queries (recorded, not modelled: compared between configurations only)
A dispatch never runs while its own Result texture is bound as the sky (a kernel that samples the image it writes has no sequential
meaning, in Unity neither), and blit_add_history never while H or N is the sky (the library refuses it): the generator keeps to that."""
import copy

import numpy as np

from unityraytracer_amd import scenes

F = np.float32
FRAME_TEX = ("T0", "T1", "C", "X0", "X1", "X2", "H", "N")
SKY_TEX = ("S0", "S1")
ALL_TEX = FRAME_TEX + SKY_TEX
FORMATS = ("RGBA32F", "RGBA8_SRGB", "RGBA16F")
KINDS = ("frame", "dispatch", "blit", "history", "setpixels", "restart", "bind_sky", "bind_result", "move_mesh", "deform", "move_spheres",
         "camera", "flush", "ptr", "get", "read_begin", "read_end", "ray_query", "radiance_query")
SUBMITTING = ("flush", "get", "read_begin", "setpixels", "ptr")   # ops that always submit the deferred frames themselves
WRITER_KINDS = ("blend", "history", "present", "blit", "dispatch", "setpixels")      # what can have written a texture last (coverage)
FRAME_SEED = 0x5EED
N_QUERIES = 64
MOVES = [dict(translate=(-1.2, 1.6, 0.4), scale=(1.2, 1.0, 0.9), yaw_deg=33.0),
         dict(translate=(-1.0, 1.5, 0.2), scale=(2.1, 0.45, 1.3), yaw_deg=-71.0),
         dict(translate=(-0.8, 1.7, 0.5), scale=(1.0, 1.0, 1.0), yaw_deg=10.0)]
SHIFTS = [(0.25, 0.0, -0.5), (-0.5, 0.25, 0.0), (0.0, -0.125, 0.75)]
CAMERA_POSITIONS = [(0.0, 1.0, -10.0), (1.5, 2.0, -9.0), (-2.0, 0.5, -11.0)]
DEFORM_SCALES = (0.75, 1.25, 0.9)


def size_class(name):
    return 1 if name in SKY_TEX else 0


# ---- the world ----------------------------------------------------------------------------------------------------------------------
def make_scene(width=64, height=40, bounces=2):
    sc = scenes.mixed_test_scene(width, height)
    sc.num_bounces, sc.num_rays = bounces, 1
    return sc


def cameras(sc):
    return [scenes.camera_matrices(sc.width, sc.height, position=p)[0] for p in CAMERA_POSITIONS]


def blob_span(sc):
    """(first, last) vertex of MeshObject 0 (the blob)."""
    mo = sc.mesh_objects[0]
    sl = np.asarray(sc.indices).reshape(-1)[int(mo["indices_offset"]): int(mo["indices_offset"]) + int(mo["indices_count"])]
    return int(sl.min()), int(sl.max())


def edited_scene(sc, op):
    """A copy of `sc` after a scene-edit op (no array of `sc` is written).  Both sides use it: it is plain host arithmetic on the lists."""
    out = copy.copy(sc)
    if op[0] == "move_mesh":
        mo = sc.mesh_objects.copy()
        mo[op[1]]["localToWorldMatrix"] = scenes.trs(**MOVES[op[2]])
        out.mesh_objects = mo
        out.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(mo, sc.vertices, sc.indices))
    elif op[0] == "deform":
        lo, hi = blob_span(sc)
        v = np.array(sc.vertices, F).reshape(-1, 3)
        part = v[lo: hi + 1]
        centre = part.mean(axis=0, dtype=np.float64).astype(F)
        v[lo: hi + 1] = (centre + (part - centre) * F(op[1])).astype(F)
        out.vertices = v
        out.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(sc.mesh_objects, v, sc.indices))
    elif op[0] == "move_spheres":
        sp = sc.spheres.copy()
        sp["position"] = (sp["position"] + np.asarray(SHIFTS[op[1]], F)).astype(F)
        out.spheres = sp
        out.sphere_bvh = scenes.build_object_bvh(*scenes.sphere_bounds(sp))
    elif op[0] == "camera":
        out.camera_to_world = cameras(sc)[op[1]]
    else:
        raise ValueError(op)
    return out


def query_rays(seed):
    """64 rays from around the scene, half of them aimed into it (fixed bounds: the edits stay within them)."""
    rng = np.random.default_rng(1000 + seed)
    lo, hi = np.array([-6.0, -1.0, -6.0]), np.array([6.0, 5.0, 6.0])
    o = (lo + rng.random((N_QUERIES, 3)) * (hi - lo)).astype(F)
    d = rng.normal(size=(N_QUERIES, 3))
    aim = np.array([-2.0, 0.0, -2.0]) + rng.random((N_QUERIES, 3)) * np.array([5.0, 3.5, 4.0]) - o
    d[: N_QUERIES // 2] = aim[: N_QUERIES // 2]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(F)


def query_pixels():
    i = np.arange(N_QUERIES, dtype=np.int64)
    return np.stack([(i % 4096).astype(F), (i // 4096).astype(F)], axis=1)


# ---- programs -----------------------------------------------------------------------------------------------------------------------
class _Track:
    """What a generator / the coverage analysis has to know about the state a program has reached."""

    def __init__(self):
        self.sky, self.result, self.tickets = "S0", "T0", 0

    def other_result(self):
        return "T1" if self.result == "T0" else "T0"

    def allowed(self, op):
        k = op[0]
        if k == "frame":
            return self.sky != self.result and op[1] != "C"
        if k == "dispatch":
            return self.sky != op[1]
        if k == "history":
            return self.sky not in ("H", "N")
        if k == "blit":
            return op[1] != op[2] and size_class(op[1]) == size_class(op[2])
        if k == "read_begin":
            return self.tickets < 2
        if k == "read_end":
            return self.tickets > 0
        return True

    def apply(self, op):
        k = op[0]
        if k == "bind_sky":
            self.sky = op[1]
        elif k == "bind_result":
            self.result = self.other_result()
        elif k == "read_begin":
            self.tickets += 1
        elif k == "read_end":
            self.tickets -= 1


def writes_of(op, result):
    """[(texture, writer kind)] of an op, in order; `result` = the Result texture bound when it runs."""
    k = op[0]
    if k == "frame":
        return [(result, "frame_dispatch"), ("C", "blend")] + ([(op[1], "present")] if op[1] else [])
    if k == "dispatch":
        return [(op[1], "dispatch")]
    if k == "blit":
        return [(op[2], "blit")]
    if k == "history":
        return [("H", "history"), ("N", "history")]
    if k == "setpixels":
        return [(op[1], "setpixels")]
    return []


_WEIGHTS = {"frame": 30, "dispatch": 5, "blit": 6, "history": 5, "setpixels": 4, "restart": 2, "bind_sky": 5, "bind_result": 3, "move_mesh": 2,
            "deform": 2, "move_spheres": 2, "camera": 2, "flush": 4, "ptr": 2, "get": 5, "read_begin": 6, "read_end": 5, "ray_query": 3,
            "radiance_query": 3}


def _draw(rng, kind, tr):
    pick = lambda names: names[int(rng.integers(len(names)))]
    if kind == "frame":
        return ("frame", pick((None, "X0", "X0", "X1", "X2", "H", tr.other_result())))
    if kind == "dispatch":
        return ("dispatch", pick(("T0", "T1")))
    if kind == "blit":
        if rng.random() < 0.25:
            return ("blit", *[SKY_TEX[i] for i in rng.permutation(2)])
        a, b = rng.permutation(len(FRAME_TEX))[:2]
        return ("blit", FRAME_TEX[a], FRAME_TEX[b])
    if kind == "history":
        return ("history", float(pick((0.0, 1.0, 4.0))))
    if kind == "setpixels":
        return ("setpixels", pick(ALL_TEX), float(pick((0.0, 0.25, 1.5))))
    if kind == "bind_sky":
        return ("bind_sky", pick((None,) + ALL_TEX))
    if kind == "move_mesh":
        return ("move_mesh", int(rng.integers(2)), int(rng.integers(len(MOVES))))
    if kind == "deform":
        return ("deform", float(pick(DEFORM_SCALES)))
    if kind == "move_spheres":
        return ("move_spheres", int(rng.integers(len(SHIFTS))))
    if kind == "camera":
        return ("camera", int(rng.integers(len(CAMERA_POSITIONS))))
    if kind == "ptr":
        return ("ptr", pick(("X0", "X1", "X2", "S1", "H")))
    if kind == "get":
        return ("get", pick(ALL_TEX))
    if kind == "read_begin":
        return ("read_begin", pick(FRAME_TEX), pick(FORMATS))
    if kind in ("ray_query", "radiance_query"):
        return (kind, int(rng.integers(1 << 16)))
    return (kind,)


def make_program(seed, n_ops=40):
    """About n_ops ops, deterministic per seed.  The plain draw is biased towards the cases the suite exists for: a texture that has just
    been written is bound as the sky and traced at once (every writer kind), readbacks and scene edits land between frames."""
    rng = np.random.default_rng(seed)
    kinds = list(_WEIGHTS)
    p = np.array([_WEIGHTS[k] for k in kinds], dtype=np.float64)
    p /= p.sum()
    tr, prog, forced = _Track(), [], []

    def emit(op):
        tr.apply(op)
        prog.append(op)

    while len(prog) < n_ops:
        if forced:
            op = forced.pop(0)
            if tr.allowed(op):
                emit(op)
            continue
        op = _draw(rng, kinds[int(rng.choice(len(kinds), p=p))], tr)
        if not tr.allowed(op):
            continue
        result = tr.result
        emit(op)
        written = [t for t, _ in writes_of(op, result) if t != tr.result]
        if op[0] == "frame":                                   # (the frame's own Result is the least interesting of what it wrote)
            written = [t for t in written if t != result] or written
        r = rng.random()
        if written and r < 0.4:                                  # written -> bound as the sky -> traced, nothing in between
            t = written[int(rng.integers(len(written)))]
            forced = [("bind_sky", t), ("frame", "X1" if t != "X1" else "X2")]
            if rng.random() < 0.5:
                forced.append(("read_begin", forced[1][1], FORMATS[int(rng.integers(3))]))
        elif op[0] in ("frame", "dispatch") and r < 0.55:        # something between two frames of what would be one batch
            mid = [("get", "C"), ("read_begin", "C", FORMATS[int(rng.integers(3))]), ("move_mesh", 0, int(rng.integers(3))), ("deform", 0.9),
                   ("move_spheres", int(rng.integers(3))), ("ray_query", 7), ("radiance_query", 7)][int(rng.integers(7))]
            forced = [mid, ("frame", None)]
    while tr.tickets:
        emit(("read_end",))
    return prog


def coverage(program):
    """Static facts about a program (tests/test_command_stream_model.py holds the seed set to them):
    kinds: op kind -> count;  sky_after: the writer kinds K for which a texture last written by K was bound as the sky AFTER that write and
    traced before anything else wrote it;  read_while_deferred: observers of an image reached while dispatches could still be deferred;
    edit_between_frames: scene edits with a dispatch before and after and nothing that submits in between."""
    kinds = {k: 0 for k in KINDS}
    tr = _Track()
    last_writer, write_at, bound_at = {}, {}, -1
    sky_after, read_deferred, edits = set(), 0, 0
    pending, edit_open = 0, False
    neutral = ("restart", "bind_sky", "bind_result", "camera")
    for i, op in enumerate(program):
        k = op[0]
        kinds[k] += 1
        if k in ("frame", "dispatch"):
            if tr.sky is not None and tr.sky in last_writer and bound_at > write_at[tr.sky]:
                sky_after.add(last_writer[tr.sky])
            if edit_open:
                edits += 1
            edit_open = False
            pending += 1
        elif k in ("move_mesh", "deform", "move_spheres"):
            edit_open = pending > 0
        elif k not in neutral:
            if k in ("get", "read_begin") and pending > 0:
                read_deferred += 1
            pending, edit_open = 0, False
        for t, w in writes_of(op, tr.result if k != "dispatch" else op[1]):
            last_writer[t], write_at[t] = w, i
        if k == "bind_sky":
            bound_at = i
        tr.apply(op)
    return {"kinds": kinds, "sky_after": sky_after, "read_while_deferred": read_deferred, "edit_between_frames": edits}


# ---- the sequential model -----------------------------------------------------------------------------------------------------------
def frame_uniforms_of(sc, frame):
    """(_PixelOffset, _Seed) RayTraceMaster.SetShaderParameters binds for its frame number `frame`."""
    if frame == 0:
        return (sc.pixel_offset[0], sc.pixel_offset[1]), sc.seed
    ox, oy, seed = scenes.frame_uniforms(frame, FRAME_SEED)
    return (ox, oy), seed


def encode(img, fmt):
    from unityraytracer_amd import host_io
    if fmt == "RGBA8_SRGB":
        return host_io.encode_srgb8(img)
    if fmt == "RGBA16F":
        with np.errstate(over="ignore"):
            return img.astype(np.float16)
    return img.copy()


def run_model(program, width=64, height=40, bounces=2, threads=8):
    """-> (observations, final contents): observations is a list of (op index, kind, array | None), final a dict name -> array."""
    from oracle import pyoracle
    from reproject_ref import blit_add_history_ref
    sc = make_scene(width, height, bounces)
    tex = {n: np.zeros((height, width, 4), F) for n in FRAME_TEX}
    tex["S0"] = np.array(sc.sky, F)
    tex["S1"] = np.zeros_like(tex["S0"])
    sky, result, sample, frame, tickets, obs = "S0", "T0", 0, 0, [], []

    def oracle():
        s = copy.copy(sc)
        s.sky = tex[sky] if sky is not None else np.zeros((1, 1, 4), F)        # an unbound texture reads zeros
        s.pixel_offset, s.seed = frame_uniforms_of(sc, frame)
        return pyoracle.Oracle(s)

    for i, op in enumerate(program):
        k = op[0]
        if k == "frame":
            tex[result] = oracle().render(mode=0, threads=threads)
            tex["C"] = pyoracle.accumulate(tex[result], tex["C"], float(sample))
            if op[1]:
                tex[op[1]] = tex["C"].copy()
            sample += 1
            frame += 1
        elif k == "dispatch":
            tex[op[1]] = oracle().render(mode=0, threads=threads)
            frame += 1
        elif k == "blit":
            tex[op[2]] = tex[op[1]].copy()
        elif k == "history":
            tex["H"], tex["N"] = blit_add_history_ref(tex[result], tex["H"], tex["N"], op[1])
        elif k == "setpixels":
            tex[op[1]] = np.full_like(tex[op[1]], F(op[2]))
        elif k == "restart":
            sample = 0
        elif k == "bind_sky":
            sky = op[1]
        elif k == "bind_result":
            result = "T1" if result == "T0" else "T0"
        elif k in ("move_mesh", "deform", "move_spheres", "camera"):
            sc = edited_scene(sc, op)
        elif k == "get":
            obs.append((i, k, tex[op[1]].copy()))
        elif k == "read_begin":
            tickets.append(encode(tex[op[1]], op[2]))
        elif k == "read_end":
            obs.append((i, k, tickets.pop(0)))
        elif k == "ray_query":
            o, d = query_rays(op[1])
            orc = oracle()
            out = np.zeros((N_QUERIES, 8), F)
            for j in range(N_QUERIES):
                r = orc.trace(o[j], d[j], mode=0)
                out[j, 0], out[j, 1:4], out[j, 4:7], out[j, 7] = r["distance"], r["position"], r["normal"], r["kind"]
            obs.append((i, k, out))
        elif k == "radiance_query":
            obs.append((i, k, None))
        elif k not in ("flush", "ptr"):
            raise ValueError(op)
    assert not tickets, "the program leaves a readback in flight"
    return obs, tex


# ---- the runner ---------------------------------------------------------------------------------------------------------------------
def run_gpu(ctx, program, frames_per_launch, overlap_launches, width=64, height=40, bounces=2):
    """The program through the Python API -> (observations, final contents, counters, [(op index, launch_info()) after every op of SUBMITTING])."""
    from unityraytracer_amd import Graphics, RayTraceMaster, RenderTexture
    ctx.set_option("kernel_mode", 3)
    ctx.set_option("frames_per_launch", frames_per_launch)
    ctx.set_option("overlap_launches", overlap_launches)
    m, tex = None, {}
    try:
        sc = make_scene(width, height, bounces)
        m = RayTraceMaster(ctx, sc, frame_seed=FRAME_SEED)
        for n in FRAME_TEX:
            tex[n] = RenderTexture(ctx, width, height)
        m._target, m._converged = tex["T0"], tex["C"]
        m._bind_for_queries()                                  # buffers, the scene's sky, the bindings
        tex["S0"] = m.SkyboxTexture
        tex["S1"] = RenderTexture(ctx, tex["S0"].width, tex["S0"].height)
        sh = m.RayTraceShader
        ctx.reset_counters()
        obs, infos, tickets = [], [], []
        gx, gy = (width + 7) // 8, (height + 7) // 8
        for i, op in enumerate(program):
            k = op[0]
            if k == "frame":
                m.OnRenderImage(tex[op[1]] if op[1] else None)
            elif k == "dispatch":
                m.SetShaderParameters()
                sh.SetTexture(0, "Result", tex[op[1]])
                sh.Dispatch(0, gx, gy, 1)
                m._frame += 1
            elif k == "blit":
                Graphics.Blit(tex[op[1]], tex[op[2]])
            elif k == "history":
                ctx.blit_add_history(m._target, tex["H"], tex["N"], op[1])
            elif k == "setpixels":
                t = tex[op[1]]
                t.SetPixels(np.full((t.height, t.width, 4), op[2], F))
            elif k == "restart":
                m._currentSample = 0
            elif k == "bind_sky":
                m.SkyboxTexture = tex[op[1]] if op[1] else None
                sh.SetTexture(0, "_SkyboxTexture", m.SkyboxTexture)
            elif k == "bind_result":
                m._target = tex["T1"] if m._target is tex["T0"] else tex["T0"]
            elif k in ("move_mesh", "deform", "move_spheres", "camera"):
                new = edited_scene(m.scene, op)
                if k == "move_mesh":
                    m._meshObjectBuffer.SetData(new.mesh_objects)
                    m._meshObjectBVHBuffer.SetData(new.mesh_bvh)
                elif k == "deform":
                    lo, hi = blob_span(new)
                    m._vertexBuffer.SetData(np.ascontiguousarray(new.vertices[lo: hi + 1]), 0, lo, hi - lo + 1)
                    m._meshObjectBVHBuffer.SetData(new.mesh_bvh)
                elif k == "move_spheres":
                    m._sphereBuffer.SetData(new.spheres)
                    m._sphereBVHBuffer.SetData(new.sphere_bvh)
                m.scene = new
            elif k == "flush":
                ctx.flush()
            elif k == "ptr":
                assert tex[op[1]].device_ptr()
            elif k == "get":
                obs.append((i, k, tex[op[1]].GetPixels()))
            elif k == "read_begin":
                tickets.append((tex[op[1]], tex[op[1]].ReadBegin(op[2])))
            elif k == "read_end":
                t, ticket = tickets.pop(0)
                obs.append((i, k, t.ReadEnd(ticket)))
            elif k == "ray_query":
                m.SetShaderParameters()
                o, d = query_rays(op[1])
                h = ctx.ray_query(o, d)
                out = np.zeros((N_QUERIES, 8), F)
                out[:, 0], out[:, 1:4], out[:, 4:7], out[:, 7] = h["distance"], h["position"], h["normal"], h["kind"]
                obs.append((i, k, out))
            elif k == "radiance_query":
                m.SetShaderParameters()
                o, d = query_rays(op[1])
                obs.append((i, k, ctx.radiance_query(o, d, query_pixels(), 0.25, 1, bounces)))
            else:
                raise ValueError(op)
            if k in SUBMITTING:                                  # (launch_info() submits what is deferred: asked only where the op has done so)
                infos.append((i, ctx.launch_info()))
        while tickets:                                           # (a program ends its own readbacks; this is for one that failed half-way)
            t, ticket = tickets.pop(0)
            t.ReadEnd(ticket)
        final = {n: t.GetPixels() for n, t in tex.items()}
        return obs, final, ctx.counters(), infos
    finally:
        ctx.set_option("frames_per_launch", 0)
        ctx.set_option("overlap_launches", 1)
        if m is not None:
            for t in tex.values():
                if t.handle:
                    t.Release()
            for name in ("_target", "_converged", "SkyboxTexture"):      # the master releases none of them twice
                t = getattr(m, name)
                if t is not None and not t.handle:
                    setattr(m, name, None)
            m.OnDisable()


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
def same(a, b):
    """Bit for bit (NaNs of any payload count as equal, as in tests/test_gpu_ray_query.py)."""
    if a is None or b is None:
        return a is None and b is None
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
        return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


def first_difference(got, want, radiance=True):
    """None, or (index of the op up to which the program matters | None = all of it, what differs first): observations in order, then the
    final contents.  radiance=False leaves the recorded radiance queries out (the model has none)."""
    obs_a, fin_a = got[0], got[1]
    obs_b, fin_b = want[0], want[1]
    if len(obs_a) != len(obs_b):
        return None, f"{len(obs_a)} observations against {len(obs_b)}"
    for n, ((i, k, a), (j, k2, b)) in enumerate(zip(obs_a, obs_b)):
        if (i, k) != (j, k2):
            return i, f"observation {n} is {k} of op {i} against {k2} of op {j}"
        if k == "radiance_query" and not radiance:
            continue
        if not same(a, b):
            bad = int(np.count_nonzero(a.reshape(-1) != b.reshape(-1)))
            return i, f"observation {n} ({k}, op {i}) differs in {bad} of {a.size} values"
    for name in fin_b:
        if not same(fin_a[name], fin_b[name]):
            return None, f"final contents of {name} differ in {int(np.count_nonzero(fin_a[name] != fin_b[name]))} of {fin_a[name].size} values"
    return None


def describe(program, upto=None):
    ops = program if upto is None else program[: upto + 1]
    return "\n".join(f"  {i:3d} {op}" for i, op in enumerate(ops))
