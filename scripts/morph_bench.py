"""Cost of blend shapes on the device (include/urt.h urt_morph_vertices, csrc/morph.hip) on a face-sized rig: 200 k vertices, 64 targets
that each touch 30 % of the vertices (3.8 M entries, 19 a vertex),
  (a) with 4 of the 64 weights live — what a frame of a real rig looks like: the kernel reads every entry's 4-byte target and the 24
      bytes of deltas of the live entries only;
  (b) with all 64 live;
  (c) urt_skin_vertices (64 bones, normals) on the same vertex count, in the same run, for scale.
Each is reported in ms and as achieved GB/s two ways: `GBps_must` over the bytes the kernel must move counting the LIVE entries only
(56 B a vertex — rest and destination rows, the range — and 28 B a live entry), `GBps_worst` over the bytes it could at worst move,
counting ALL entries.  If (a) is not faster than (b), reading the deltas only when live did not pay and the packed layout should be
kept instead: the script says so.  The plan (107 MB) fits the chip's 256 MB last-level cache: these are warm-cache rates.

Times are a host clock around a window of --reps calls that ends in a synchronise, --repeats windows per case with the cases
alternating, medians: a call of a few microseconds (the skin at this size) is then bound by the rate at which launches can be issued,
not by the kernel.

    python scripts/morph_bench.py [--vertices 200000] [--targets 64] [--touch 0.3] [--live 4] [--reps 2000] [--repeats 5] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before the library: one HIP runtime in the process, tests/conftest.py)

from unityraytracer_amd import ComputeBuffer, Context, _lib  # noqa: E402

F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=200000)
    ap.add_argument("--targets", type=int, default=64)
    ap.add_argument("--touch", type=float, default=0.3)
    ap.add_argument("--live", type=int, default=4)
    ap.add_argument("--reps", type=int, default=2000, help="calls per timed window (a host clock around the window, which ends in a synchronise)")
    ap.add_argument("--repeats", type=int, default=5, help="windows per case, the cases alternating; medians are reported")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, nt = args.vertices, args.targets
    rng = np.random.default_rng(0)
    target, vertex = np.nonzero(rng.random((nt, n)) < args.touch)
    d = np.zeros(len(vertex), dtype=np.dtype(_lib.MORPH_DELTA_DT))
    d["vertex"], d["target"] = vertex, target
    d["dp"], d["dn"] = rng.uniform(-0.1, 0.1, (len(d), 3)).astype(F), rng.uniform(-0.1, 0.1, (len(d), 3)).astype(F)
    per_target = np.bincount(target, minlength=nt)
    results = []
    with Context(0) as ctx:
        t0 = time.perf_counter()
        plan = ctx.morph_plan(d, nt, 0, n)
        plan_ms = (time.perf_counter() - t0) * 1e3
        info = plan.info()
        bufs = {k: ComputeBuffer(ctx, n, s) for k, s in (("rest_v", 12), ("rest_n", 12), ("idx", 16), ("wgt", 16), ("dst_v", 12), ("dst_n", 12))}
        bufs["rest_v"].SetData(rng.uniform(-1, 1, (n, 3)).astype(F)); bufs["rest_n"].SetData(rng.normal(size=(n, 3)).astype(F))
        weights = ComputeBuffer(ctx, nt, 4)

        def timed(fn):
            for _ in range(3):
                fn()
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.reps

        def morph():
            plan.morph(bufs["rest_v"], bufs["rest_n"], weights, bufs["dst_v"], bufs["dst_n"], normalize=True)

        base = {"vertices": n, "targets": nt, "entries": info["n_entries"], "max_valence": info["max_valence"], "plan_device_MB": round(info["device_bytes"] / 1e6, 1),
                "plan_create_ms": round(plan_ms, 1), "reps_per_window": args.reps, "windows": args.repeats}
        n_bones = 64
        bones = ComputeBuffer(ctx, n_bones, 48)
        bones.SetData(rng.uniform(-1, 1, (n_bones, 12)).astype(F))
        bufs["idx"].SetData(rng.integers(0, n_bones, (n, 4)).astype(np.int32)); bufs["wgt"].SetData(rng.uniform(0, 1, (n, 4)).astype(F))
        few_name = "morph_%d_live" % args.live
        tables = {}
        for name, live in ((few_name, args.live), ("morph_all_live", nt)):
            w = np.zeros(nt, F)
            w[rng.permutation(nt)[:live]] = rng.uniform(0.2, 1.0, live).astype(F)
            tables[name] = w
        ms_of = {few_name: [], "morph_all_live": [], "skin_64_bones_normals": []}
        for _ in range(args.repeats):                         # the three cases alternate: a drift of the machine shows in all of them
            for name in (few_name, "morph_all_live"):
                weights.SetData(tables[name])
                ms_of[name].append(timed(morph))
            ms_of["skin_64_bones_normals"].append(timed(
                lambda: ctx.skin_vertices(bufs["rest_v"], bufs["rest_n"], bufs["idx"], bufs["wgt"], bones, 0, n, bufs["dst_v"], bufs["dst_n"])))
        for name in (few_name, "morph_all_live"):
            live_entries = int(per_target[tables[name] != 0].sum())
            must, worst = 56 * n + 28 * live_entries, 56 * n + 28 * info["n_entries"]
            ms = float(np.median(ms_of[name]))
            r = dict(base, case=name, live_targets=int((tables[name] != 0).sum()), live_entries=live_entries, ms=round(ms, 4),
                     ms_runs=[round(x, 4) for x in ms_of[name]], must_MB=round(must / 1e6, 1), worst_MB=round(worst / 1e6, 1),
                     GBps_must=round(must / (ms * 1e-3) / 1e9, 1), GBps_worst=round(worst / (ms * 1e-3) / 1e9, 1))
            print(json.dumps(r), flush=True); results.append(r)
        ms = float(np.median(ms_of["skin_64_bones_normals"]))
        r = {"case": "skin_64_bones_normals", "vertices": n, "ms": round(ms, 4), "ms_runs": [round(x, 4) for x in ms_of["skin_64_bones_normals"]],
             "must_MB": round(80 * n / 1e6, 1), "GBps_must": round(80 * n / (ms * 1e-3) / 1e9, 1)}
        print(json.dumps(r), flush=True); results.append(r)
        few, every = float(np.median(ms_of[few_name])), float(np.median(ms_of["morph_all_live"]))
        verdict = {"case": "verdict", "few_live_over_all_live": round(few / every, 3),
                   "reading_deltas_only_when_live": "pays" if few < every else "DOES NOT PAY: keep the packed layout instead"}
        print(json.dumps(verdict), flush=True); results.append(verdict)
        plan.Release(); bones.Release(); weights.Release()
        for b in bufs.values():
            b.Release()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
