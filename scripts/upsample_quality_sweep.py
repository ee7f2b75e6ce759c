"""The thresholds of urt_upsample swept on the set-up of tests/test_gpu_upsample.py::test_quality_at_edges_beats_a_plain_bilinear_resize
(a measurement, not a test): mixed scene, 48 x 32 traced for 16 or 256 frames under three seeds, against 96 x 64 traced for 64 or 1024
frames; RMSE over the pixels within 2 texels of an id or kind change, for the plain bilinear resize and for the guided result under each
(normal_threshold, plane_threshold, wide_fallback, sky_from_albedo), whole mask / sky pixels / surface pixels / surface pixels that got a
result.  DESIGN.md §22 quotes it; profiles/r19_logs/quality_thresholds.log is its output.

    python scripts/upsample_quality_sweep.py
"""
import itertools
import os
import sys

import torch  # noqa: F401  (before the library: one HIP runtime in the process, tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from upsample_ref import bilinear_resize_ref
from test_gpu_upsample import edge_mask
from unityraytracer_amd import Context, RayTraceMaster, scenes
from unityraytracer_amd.unity_api import RenderTexture

W, H = 96, 64
with Context(0) as ctx:
    truths = {}
    for frames in (64, 1024):
        tm = RayTraceMaster(ctx, scenes.mixed_test_scene(W, H), frame_seed=0xBEEF)
        for _ in range(frames):
            tm.OnRenderImage()
        truths[frames] = tm._converged.GetPixels()[..., :3].astype(np.float64)
        tm.OnDisable()
    print("numRays", scenes.mixed_test_scene(W, H).num_rays, "truth max", truths[64].max(), "truth mean", truths[64].mean())
    for seed, low_frames in itertools.product((0x5EED, 0x1234, 0x77), (16, 256)):
        m = RayTraceMaster(ctx, scenes.mixed_test_scene(48, 32), frame_seed=seed)
        for _ in range(low_frames):
            m.OnRenderImage()
        m.Upscale(W, H)
        low = m._converged.GetPixels()
        low_hit, low_normal, _, low_id = m._uplow
        hit, normal, albedo, ids = m._upaov
        idp, nrp = ids.GetPixels(), normal.GetPixels()
        mask = edge_mask(idp, nrp, 2)
        sky = nrp[..., 3] == 0
        plain = bilinear_resize_ref(low, W, H)[..., :3]
        out, cnt = RenderTexture(ctx, W, H), RenderTexture(ctx, W, H)
        for tf in (64, 1024):
            truth = truths[tf]
            def rmse(a, sel):
                return float(np.sqrt(((a[..., :3].astype(np.float64) - truth)[sel] ** 2).mean()))
            print(f"seed {seed:#x} low_frames {low_frames} truth_frames {tf}: mask {int(mask.sum())} (sky {int((mask & sky).sum())}) "
                  f"plain all {rmse(plain, mask):.4f} sky {rmse(plain, mask & sky):.4f} surf {rmse(plain, mask & ~sky):.4f}")
            for nt, pt, wide, sfa in [(0.9, 0.02, True, True), (0.9, 0.02, True, False), (0.9, 0.02, False, True), (0.8, 0.02, True, True),
                                      (0.7, 0.02, True, True), (0.5, 0.02, True, True), (0.0, 0.02, True, True), (-1.0, 0.02, True, True),
                                      (0.9, 0.05, True, True), (0.9, 0.2, True, True), (0.9, 1e9, True, True), (0.5, 0.1, True, True),
                                      (0.0, 0.2, True, True), (-1.0, 1e9, True, True), (0.7, 0.1, True, True)]:
                ctx.upsample(m._converged, low_hit, low_normal, low_id, hit, normal, ids, out, cnt, albedo=albedo, sky_from_albedo=sfa,
                             normal_threshold=nt, plane_threshold=pt, wide_fallback=wide)
                g, c = out.GetPixels(), cnt.GetPixels()[..., 0]
                holes = c == 0
                print(f"   nt {nt:5.2f} pt {pt:8.2g} wide {int(wide)} sky_albedo {int(sfa)}: all {rmse(g, mask):.4f} sky {rmse(g, mask & sky):.4f} "
                      f"surf {rmse(g, mask & ~sky):.4f} surf-no-holes {rmse(g, mask & ~sky & ~holes):.4f} (plain there {rmse(plain, mask & ~sky & ~holes):.4f}) "
                      f"holes {int(holes.sum())} in mask {int((holes & mask).sum())}")
        out.Release(); cnt.Release()
        m.OnDisable()
