"""Off the GPU: the decision logic of the tile entry table (csrc/tile_entry.h — the frustum of a tile, the plane and cone tests that
drop a child, the frontier under its budget and stack bound, the record a lane reads) run by tests/tile_entry_main.cpp, a program with its
own main, compiled here by g++ -fsanitize=address,undefined with the sanitizer runtimes linked statically and run in the environment as it
is.  For small random meshes, near, far from the origin and along the axes, and K = 1, 2, 4, 8: the walk from a tile's list returns the
(t, u, v, triangle) bits of the walk from the root for rays anywhere in the tile, and never uses more stack.  Nothing is loaded into this
process."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walks_from_the_lists_equal_walks_from_the_root_and_the_code_runs_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "tile_entry_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "tile_entry_main.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "tile entry lists: ok" in run.stdout, run.stdout + run.stderr
