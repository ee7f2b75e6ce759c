# GPU: urt_debug_launch_info and the statistics of the tile entry table (option "tile_entry") for C3 and C3D at 1920x1080, 64 frames per launch
import sys
sys.path.insert(0, '.')
import numpy as np
from unityraytracer_amd import Context, RayTraceMaster, scenes
ctx = Context(0)
for cfg in ("C3", "C3D"):
    sc = scenes.CONFIGS[cfg]()
    m = RayTraceMaster(ctx, sc)
    for _ in range(64):
        m.OnRenderImage()
    ctx.synchronize()
    info = ctx.launch_info()
    table, builds = ctx.read_tile_entry()
    n = (table != -2 ** 31).sum(axis=2)
    si = ctx.scene_info()
    nodes = ctx.read_scene_blas(1)[0]
    print(cfg, {k: info[k] for k in ("kernel", "n_frames", "lds_bytes", "top_nodes", "blas_stack", "waves_per_cu", "tile_entry", "tile_entry_k")}, "scene", si)
    print(cfg, "tiles", table.shape, "builds", builds, "entries per tile: mean %.2f" % n.mean(), "histogram", np.bincount(n.reshape(-1), minlength=9).tolist(),
          "first entry below the LDS top (>= top_nodes or a leaf): %.3f of the non-empty tiles" % ((table[..., 0][n > 0] >= info["top_nodes"]) | (table[..., 0][n > 0] < 0)).mean())
    m.OnDisable()
