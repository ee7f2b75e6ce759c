"""Cost of a full preparation whose geometry lives in device memory (include/urt.h option "prepare_device"): the download path (the
default: _Vertices / _Indices / _Normals come down, and a GPU builder sends them straight back up) against the device-fed path (a
device-to-device copy, the build, the vertex spans from csrc/index_span.hip).

For C3 (69,600 triangles) and C5 (983,040): all three geometry buffers are written with SetDataDevice from torch tensors, _Indices with the
triangle order of the first MeshObject rotated by one against the previous step — same surface, but a full preparation follows.  One
step = the three SetDataDevice calls, a dispatch and synchronize (host wall clock: `step_ms`); `prepare_ms` is urt_debug_scene_info's
host time of the preparation inside it.  Median and min .. max of `--repeats` steps after `--warmup`, the modes of one scene
interleaved step by step.  Modes: "blas_builder" 3 with "prepare_device" 0 and 1 (only the transfer path differs), and the default builder
(-1) with both.  A library that does not know the option (the parent commit's, through URT_LIB_PATH) runs the download modes only.
A last pass with "time_dispatch" on reads the span kernel's device time (urt_debug_prepare_stats) and holds its bytes per second
against a device-to-device copy of the same bytes (torch's copy_ of a contiguous tensor: hipMemcpyAsync DtoD), timed with events in the same run.

    [URT_LIB_PATH=old.so] python scripts/device_prepare_bench.py [--configs C3,C5] [--repeats 20] [--warmup 5] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime in the process, tests/conftest.py)

from unityraytracer_amd import Context, RayTraceMaster, scenes  # noqa: E402
from unityraytracer_amd._lib import UrtError  # noqa: E402

SIZE = (256, 144)                                          # the frame is not what is measured: a small one


def summary(name, ms):
    return {name + "_median": round(float(np.median(ms)), 3), name + "_min": round(float(min(ms)), 3), name + "_max": round(float(max(ms)), 3)}


class Mode:
    """One context that regenerates its geometry on the device every step."""

    def __init__(self, sc, tensors, builder, device, timed=False):
        self.name = f"builder{builder}_device{device}"
        self.ctx = Context(0)
        self.known = True
        self.ctx.set_option("blas_builder", builder)
        try:
            self.ctx.set_option("prepare_device", device)
        except UrtError:
            self.known = device == 0                         # an older library: only the download path exists
        if timed:
            self.ctx.set_option("time_dispatch", 1)
        self.tv, self.ti, self.tn = tensors
        self.steps, self.prep, self.span = [], [], []
        if self.known:
            self.m = RayTraceMaster(self.ctx, sc)
            self.m.OnRenderImage()
            self.ctx.synchronize()

    def step(self, k, keep):
        ctx, m = self.ctx, self.m
        ctx.synchronize()
        t0 = time.perf_counter()
        m._vertexBuffer.SetDataDevice(self.tv)
        m._indexBuffer.SetDataDevice(self.ti[k % 2])
        m._normalBuffer.SetDataDevice(self.tn)
        m._frame = 0; m._currentSample = 0
        m.OnRenderImage()
        ctx.synchronize()
        t1 = time.perf_counter()
        if keep:
            self.steps.append((t1 - t0) * 1e3)
            self.prep.append(ctx.scene_info()["prepare_ms"])
            if hasattr(ctx.lib, "urt_debug_prepare_stats"):
                self.span.append(ctx.prepare_stats()["span_ms"])

    def downloads(self):
        m = self.m
        return [self.ctx.buffer_state(b)["downloads"] for b in (m._vertexBuffer, m._indexBuffer, m._normalBuffer)]

    def close(self):
        if self.known:
            self.m.OnDisable()
        self.ctx.close()


def copy_ms(n_bytes, repeats, warmup):
    """Device time of a device-to-device copy of n_bytes, per repeat."""
    src = torch.arange(n_bytes // 4, dtype=torch.int32, device="cuda")
    dst = torch.empty_like(src)
    out = []
    for k in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,C5")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("device_prepare_bench: no GPU (there is nothing to measure without one)")
    tag = os.environ.get("URT_LIB_PATH") or "this tree"
    results = []
    for cfg in args.configs.split(","):
        sc = scenes.CONFIGS[cfg](*SIZE)
        n0 = int(sc.mesh_objects[0]["indices_count"]) // 3 * 3
        off = int(sc.mesh_objects[0]["indices_offset"])
        rolled = sc.indices.copy()
        rolled[off: off + n0] = np.roll(sc.indices[off: off + n0].reshape(-1, 3), 1, axis=0).reshape(-1)
        cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        tensors = (cuda(sc.vertices), (cuda(sc.indices), cuda(rolled)), cuda(sc.normals))
        modes = [Mode(sc, tensors, b, d) for b, d in ((3, 0), (3, 1), (-1, 0), (-1, 1))]
        modes = [mo for mo in modes if mo.known or mo.close()]
        for k in range(args.warmup + args.repeats):
            for mo in modes:                                 # interleaved: what else runs on the machine meets every mode alike
                mo.step(k, k >= args.warmup)
        for mo in modes:
            r = {"lib": tag, "config": cfg, "triangles": sc.n_triangles, "meshes": len(sc.mesh_objects), "mode": mo.name,
                 "builder_ran": mo.ctx.launch_info()["blas_builder"], "repeats": args.repeats, "downloads_v_i_n": mo.downloads(),
                 "geometry_bytes": int(sc.vertices.nbytes + sc.indices.nbytes + sc.normals.nbytes)}
            r.update(summary("step_ms", mo.steps))
            r.update(summary("prepare_ms", mo.prep))
            print(json.dumps(r), flush=True)
            results.append(r)
            mo.close()
        timed = Mode(sc, tensors, 3, 1, timed=True)          # the span kernel alone, by events around it
        if timed.known:
            for k in range(args.warmup + args.repeats):
                timed.step(k, k >= args.warmup)
            scanned = int(sum(int(c) // 3 * 3 for c in sc.mesh_objects["indices_count"])) * 4
            cp = copy_ms(scanned, args.repeats, args.warmup)
            span, copy = float(np.median(timed.span)), float(np.median(cp))
            r = {"lib": tag, "config": cfg, "mode": "span_kernel", "scanned_bytes": scanned, "chunk": timed.ctx.prepare_stats()["span_chunk"]}
            r.update(summary("span_ms", timed.span))
            r.update(summary("copy_ms", cp))
            r["span_GBps"] = round(scanned / span / 1e6, 1) if span > 0 else None
            r["copy_GBps_read"] = round(scanned / copy / 1e6, 1) if copy > 0 else None
            r["span_rate_over_copy_rate"] = round(copy / span, 3) if span > 0 else None
            print(json.dumps(r), flush=True)
            results.append(r)
        timed.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
