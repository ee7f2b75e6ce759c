#!/usr/bin/env python3
"""Where the VALU instructions of one k_sched instantiation sit, by instruction class, and what their mix costs per instruction.

    python3 scripts/valu_attribution.py [--kernel 'k_sched<false, 256, 0, false, false>'] [-DURT_... ...]

Compiles csrc/kernels.hip to assembly with build.py's flags plus line tables (--cuda-device-only -S -gline-tables-only) and walks the
kernel's instruction stream.  Every VALU instruction is put into one of the classes of the issue-rate table
(profiles/r03_logs/r3_valu_table_microbench.log), in SIMD cycles per wave-instruction:
    fast  2.5   v_fma / v_mul / v_add / v_sub / v_mov f32, v_and / v_or / v_xor
    slow  4.4   min / max / compares / v_cndmask / conversions / shifts and integer adds / readlane
    imul  4.4   v_mul_lo / v_mul_hi / v_mad_u64_u32 (the table has v_mul_lo_u32 at 4.43; counted apart because a division is made of them)
    trans 8.4   v_rcp / v_rsq / v_sqrt / v_div_* and the other quarter-rate operations
(the table's column for eight waves per SIMD: the issue cost)
and attributed to a GROUP of device functions through its .loc line (the function whose definition precedes the line in its header;
instructions of include/urt_math.h, which everything calls, go to the group of the last instruction before them that was not).  The
attribution is by position in the stream: the scheduler interleaves neighbours, so read the groups to a few per cent, not to the
instruction.  Output: per basic block the counts and the group; per group the static counts and what the static mix would cost per
instruction.  STATIC only: a group's blocks do not all run on every trip, so static counts times the trips per wave of scripts/stamps3.py
overshoot a wave's executed instructions (threefold on C3) — shares of the executed instructions need per-block execution counts, which
this script does not have."""
import collections, os, re, shutil, subprocess, sys, tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from unityraytracer_amd.build import CSRC, HIPCC_FLAGS

CYCLES = {"fast": 2.5, "slow": 4.4, "imul": 4.4, "trans": 8.4}        # eight waves per SIMD: the issue cost
GROUPS = [   # (group, functions) — the first match wins; whatever is left in kernels.hip is the scheduler loop itself
    ("handout", "wg_fetch_pixels wg_fetch_run wave_fetch_pixels slot_pixel shard_slots shard_tile wave_uniform64 run_word launch_tiles"),
    ("camera", "camera_ray_frame camera_ray_uv camera_ray mul_m4_k axis_uv jitter_uv kernarg_floats for_each_frame"),
    ("shade", "shade_surface sample_hemisphere shade"),
    ("sky", "shade_sky sky_radiance sample_sky sky_texel"),
    ("leaf", "test_leaf tri_test intersect_triangle"),
    ("node", "blas_node_eval_cone_ptr blas_node_eval_ptr blas_node_eval blas_node_select_ptr cone_skips cone_ray_word blas_ray qnode_eval_ptr make_qray"),
    ("front", "front_single trace_front front_listed front_masked ground_plane intersect_sphere tlas_slab tlas_slab_t"),
    ("flush", "flush_counters wave_sum report_watchdog"),
]
BY_FILE = {"kernels.hip": "sched", "front_device.h": "front", "sky_device.h": "sky", "shade_device.h": "shade", "camera_device.h": "camera"}


def classify(op):
    if re.match(r"v_(mul_lo|mul_hi|mad_u64|mad_i64)", op): return "imul"
    if re.match(r"v_(rcp|rsq|sqrt|div_|exp|log|sin|cos)", op): return "trans"
    if re.match(r"v_(fma|fmac|mul|add|sub|subrev|mov|mac|mad)_(f32|legacy_f32|b32)|v_(and|or|xor|not)_b32|v_bitop3", op): return "fast"
    return "slow"


def function_starts(path):
    out = []
    for n, line in enumerate(open(path, errors="replace"), 1):
        m = re.match(r"\s*(?:template\s*<[^>]*>\s*)?(?:__device__|__global__|URT_HD|static|inline)[^;(]*?\b(\w+)\s*\(", line)
        if m: out.append((n, m.group(1)))
    return out


def main(argv):
    kernel, defines = "k_sched<false, 256, 0, false, false>", []
    it = iter(argv)
    for a in it:
        if a == "--kernel": kernel = next(it)
        else: defines.append(a)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    flags = [f for f in HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + defines + ["--cuda-device-only", "-S", "-gline-tables-only"]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "kernels.s")
        subprocess.run([hipcc] + flags + [os.path.join(CSRC, "kernels.hip"), "-o", out], check=True)
        text = open(out).read().splitlines()
    files, starts = {}, {}
    for line in text:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', line)
        if m:
            path = os.path.join(m.group(2), m.group(3)) if m.group(3) else m.group(2)
            files[int(m.group(1))] = path
    group_of = {f: g for g, fs in GROUPS for f in fs.split()}

    def owner(fileno, lineno):
        path = files.get(fileno, "")
        base = os.path.basename(path)
        if base == "urt_math.h" or "csrc" not in path: return None   # urt_math.h, the HIP headers: the group of what came before
        if path not in starts: starts[path] = function_starts(path) if os.path.exists(path) else []
        fn = None
        for n, name in starts[path]:
            if n > lineno: break
            fn = name
        return group_of.get(fn) or BY_FILE.get(base)               # (None: a small helper of trace_device.h / frame_device.h — the group of what came before)

    mangled = None
    for line in text:                                              # the label whose demangled name is the kernel's
        m = re.match(r"^(_Z\w+):", line)
        if m and "k_sched" in m.group(1):
            name = subprocess.run(["c++filt", "-p", m.group(1)], capture_output=True, text=True).stdout.strip()
            if name.endswith(kernel): mangled = m.group(1); break
    if not mangled: sys.exit(f"no kernel {kernel} in kernels.hip")
    at = next(i for i, line in enumerate(text) if line.startswith(mangled + ":"))
    blocks, cur, grp = [], None, "sched"
    salu = 0
    for line in text[at + 1:]:
        s = line.strip()
        if s.startswith(".Lfunc_end"): break
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            g = owner(int(m.group(1)), int(m.group(2)))
            if g: grp = g
            continue
        if re.match(r"^\.?\w+:", s) and not s.startswith(".loc"):
            cur = {"label": s.split(":")[0], "n": collections.Counter(), "g": collections.Counter()}; blocks.append(cur); continue
        if cur is None: cur = {"label": "entry", "n": collections.Counter(), "g": collections.Counter()}; blocks.append(cur)
        op = s.split()[0] if s and not s.startswith((";", ".")) else ""
        if op.startswith("v_"):
            c = classify(op); cur["n"][c] += 1; cur["g"][(grp, c)] += 1
        elif op.startswith("s_"): salu += 1
    per_group = collections.defaultdict(collections.Counter)
    print(f"# {kernel}: basic blocks with VALU instructions (label, fast, slow, imul, trans, groups)")
    for b in blocks:
        if not sum(b["n"].values()): continue
        gs = collections.Counter()
        for (g, c), n in b["g"].items(): gs[g] += n; per_group[g][c] += n
        print(f"{b['label']:14s} {b['n']['fast']:5d} {b['n']['slow']:5d} {b['n']['imul']:4d} {b['n']['trans']:4d}   " + " ".join(f"{g}:{n}" for g, n in gs.most_common(3)))
    tot = collections.Counter()
    print(f"\n# per group, static (fast slow imul trans | total | cycles at the table's rates | cycles per instruction)")
    for g, n in sorted(per_group.items(), key=lambda kv: -sum(kv[1].values())):
        tot.update(n)
        cyc = sum(CYCLES[c] * k for c, k in n.items()); k = sum(n.values())
        print(f"{g:28s} {n['fast']:5d} {n['slow']:5d} {n['imul']:4d} {n['trans']:4d} | {k:5d} | {cyc:8.1f} | {cyc / k:4.2f}")
    k = sum(tot.values()); cyc = sum(CYCLES[c] * v for c, v in tot.items())
    print(f"{'all':28s} {tot['fast']:5d} {tot['slow']:5d} {tot['imul']:4d} {tot['trans']:4d} | {k:5d} | {cyc:8.1f} | {cyc / k:4.2f}     (SALU {salu})")


if __name__ == "__main__":
    main(sys.argv[1:])
