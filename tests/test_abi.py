"""The C-ABI library loads, exports every symbol include/urt.h declares, and refuses to work without a GPU
(no CPU fallback).  No compute entry point is called here."""
import ctypes as C
import os
import re

import pytest

import unityraytracer_amd as urt
from unityraytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, "include", "urt.h")).read()
    return sorted(set(re.findall(r"URT_API\s+[\w\s\*]+?\b(urt_\w+)\s*\(", text)))


def test_header_and_binding_agree():
    assert header_symbols() == sorted(_lib.ABI_SYMBOLS)


def test_csharp_binding_declares_every_entry_point():
    """integration/UrtNative.cs is source only (no C# toolchain in this image): at least it must name every entry point of the header
    in a [DllImport] declaration, and nothing the header does not have."""
    text = open(os.path.join(ROOT, "integration", "UrtNative.cs")).read()
    declared = set(re.findall(r"\[DllImport\(Lib\)\]\s+internal static extern [\w\[\]]+ (urt_\w+)\(", text))
    assert declared == set(header_symbols()), (sorted(set(header_symbols()) - declared), sorted(declared - set(header_symbols())))


def test_library_exports_every_declared_symbol(built_library):
    lib = C.CDLL(built_library)
    for name in header_symbols():
        assert hasattr(lib, name), f"{name} is declared in include/urt.h but not exported"
    assert _lib.load().urt_abi_version() == 4          # positive: the product build (negative = an experiment build, below)


def test_experiment_switches_are_quarantined():
    """Every A/B / probe / diagnostic compile-time switch of csrc/ sits behind csrc/experiments.h: a translation unit that sees one
    without -DURT_EXPERIMENT does not compile, an experiment build reports a negative ABI version, and _lib.load() refuses such a
    library unless the caller opts in (URT_ALLOW_EXPERIMENT=1: scripts/ only)."""
    csrc = os.path.join(ROOT, "unityraytracer_amd", "csrc")
    guard = open(os.path.join(csrc, "experiments.h")).read()
    used = set()
    for f in os.listdir(csrc):
        if f != "experiments.h":
            used |= set(re.findall(r"#\s*if(?:n?def|\s+defined\(?)\s*(URT_[A-Z0-9_]+)", open(os.path.join(csrc, f)).read()))
    used -= {"URT_EXPERIMENT"}
    assert used, "no switches found: the scan is broken"
    for name in used:
        assert f"defined({name})" in guard, f"{name} is a compile-time switch that csrc/experiments.h does not guard"
    sources = {f for f in os.listdir(csrc) if f.endswith((".cpp", ".hip")) and '#include "experiments.h"' in open(os.path.join(csrc, f)).read()}
    assert {"scene_prep.cpp", "frame_batch.cpp", "image_ops.cpp", "geometry_ops.cpp"} <= sources       # the files context.cpp was split into
    for src in sorted(sources | {"kernels.hip", "kernels_basic.hip", "kernels_serve.hip", "kernels_pool.hip", "context.cpp", "blas_builder.cpp"}):
        head = open(os.path.join(csrc, src)).read()
        first_include = re.search(r'^#include\s+[<"]([^">]+)[">]', head, re.M).group(1)
        assert first_include == "experiments.h", (src, first_include)
    assert "URT_ABI_SIGN * " in open(os.path.join(csrc, "context.cpp")).read()
    # the loader's side: a library whose urt_abi_version() is negative is refused (checked on the logic, no second build needed)
    text = open(os.path.join(ROOT, "unityraytracer_amd", "_lib.py")).read()
    assert "urt_abi_version() < 0" in text and "URT_ALLOW_EXPERIMENT" in text


def test_layout_strides_match_reference():
    # RayTraceMaster.cs:42-45
    assert urt.scenes.PARAMS_DT.itemsize == 40 and urt.scenes.MESHOBJECT_DT.itemsize == 112
    assert urt.scenes.SPHERE_DT.itemsize == 56 and urt.scenes.BVHNODE_DT.itemsize == 28
    assert urt.scenes.MESHOBJECT_DT.fields["indices_offset"][1] == 64 and urt.scenes.MESHOBJECT_DT.fields["lighting"][1] == 72
    assert urt.scenes.SPHERE_DT.fields["radius"][1] == 12 and urt.scenes.BVHNODE_DT.fields["index"][1] == 24


def test_no_cpu_fallback(built_library):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(urt.UrtError) as e:
        urt.Context(0)
    assert e.value.code == 3 and "no CPU fallback" in str(e.value)      # URT_ERR_NO_DEVICE


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(ImportError):
        _lib.load()


def test_product_never_touches_the_oracle():
    """The shipped path must not import, include, link or load anything under oracle/ (comments may cite it)."""
    pkg = os.path.join(ROOT, "unityraytracer_amd")
    bad = re.compile(r"import\s+oracle|from\s+oracle|pyoracle|liboracle|#include\s*[\"<][^\">]*oracle|dlopen[^\n]*oracle")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not bad.search(text), f"{f} references the oracle"
    for f in os.listdir(os.path.join(ROOT, "include")):
        assert not bad.search(open(os.path.join(ROOT, "include", f)).read()), f


def test_only_the_holders_allocate_and_create():
    """csrc/owned.h is the one place that takes a GPU resource and gives it back: every other file of csrc/ reaches device memory, pinned
    memory, events and streams through its holders, so that a destroyed context or group leaks nothing (tests/test_gpu_resources.py)
    and urt_debug_live_resources counts everything.  Comments and string literals may name the calls."""
    calls = ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree(", "hipEventCreate", "hipEventDestroy(", "hipStreamCreate", "hipStreamDestroy(")
    csrc = os.path.join(ROOT, "unityraytracer_amd", "csrc")
    strip = re.compile(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"', re.S)
    code = {f: strip.sub(" ", open(os.path.join(csrc, f)).read()) for f in sorted(os.listdir(csrc))}
    assert len(code) > 40 and "owned.h" in code
    for c in calls:
        assert c in code["owned.h"], f"the scan does not find {c} in owned.h"
    found = [(f, c) for f, text in code.items() if f != "owned.h" for c in calls if c in text]
    assert not found, found


def test_header_is_plain_c99_and_the_c_example_compiles(tmp_path):
    """include/urt.h is the drop-in boundary: it must parse as C (not only C++), warning-free, and examples/frame_loop.c — the
    reference's frame protocol written in C99 against it — must compile (linking/running it needs the GPU: tests/test_gpu_c_host.py)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    inc = "-I" + os.path.join(root, "include")
    (tmp_path / "only_header.c").write_text('#include "urt.h"\nint urt_header_probe(void) { return (int)sizeof(urt_counters); }\n')
    for std in ("-std=c99", "-std=c11"):
        subprocess.run(["gcc", std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", inc, str(tmp_path / "only_header.c")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "frame_loop.c")], check=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, "-x", "c++", str(tmp_path / "only_header.c")], check=True)
