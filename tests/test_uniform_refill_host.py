"""Off the GPU: what the host puts into a batched launch's frame table (csrc/frame_derived.h: the seed-only halves of a pixel's first two
rand() draws, the camera ray's origin) equals, as bit patterns, what include/urt_math.h gives per lane for the same inputs — checked by
tests/frame_derived_main.cpp, a program with its own main, compiled here by g++ -fsanitize=address,undefined with the sanitizer
runtimes linked statically and run in the environment as it is.  Nothing is loaded into this process."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_frame_table_values_are_the_per_lane_ones_and_the_code_runs_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "frame_derived_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "frame_derived_main.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "frame table: ok" in run.stdout, run.stdout + run.stderr
