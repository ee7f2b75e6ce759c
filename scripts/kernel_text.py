#!/usr/bin/env python3
"""One line per GPU kernel of the product: demangled name (without the parameter list), sha256 of its instruction bytes, its kernel-descriptor settings.

    python3 scripts/kernel_text.py [-DURT_EXPERIMENT -DURT_STAMPS ...] > listing.txt

Compiles the device code object of every .hip in build.py's SOURCES with build.py's flags (plus the -D given) and lists what
is in it.  A kernel's machine code depends only on the text it includes (everything is inlined), so two trees whose listings
`diff` empty run the same device code, wherever a kernel sits in its file or in which file: the proof a code move needs, on a
machine without a GPU (profiles/r12_logs/README.md).  The descriptor's code-entry offset is left out: it is the kernel's position.
It hashes and lists; it does not look into the code."""
import hashlib, os, shutil, struct, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from unityraytracer_amd.build import CSRC, HIPCC_FLAGS, SOURCES


def kernels(path):
    """(mangled name, instruction bytes, descriptor fields) of every kernel in the ELF code object at `path`."""
    elf = open(path, "rb").read()
    shoff, shentsize, shnum = struct.unpack_from("<Q", elf, 0x28)[0], *struct.unpack_from("<HH", elf, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]     # name, type, flags, addr, offset, size, link, ...
    symtab = next(s for s in sec if s[1] == 2)
    strtab = sec[symtab[6]]
    syms = {}
    for at in range(symtab[4], symtab[4] + symtab[5], 24):
        name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, at)
        end = elf.index(b"\0", strtab[4] + name)
        syms[elf[strtab[4] + name:end].decode()] = (info & 15, shndx, value, size)

    def data(sym):
        _, shndx, value, size = sym
        at = sec[shndx][4] + value - sec[shndx][3]
        return elf[at:at + size]

    for name, sym in syms.items():
        if sym[0] == 2 and name + ".kd" in syms:                    # STT_FUNC with a kernel descriptor
            kd = data(syms[name + ".kd"])
            lds, scratch, kernarg = struct.unpack_from("<III", kd, 0)
            rsrc3, rsrc1, rsrc2, props, dyn_stack = struct.unpack_from("<IIIHH", kd, 44)     # (bytes 16..23, the code-entry offset, left out)
            yield name, data(sym), f"lds={lds} scratch={scratch} kernarg={kernarg} rsrc1={rsrc1:#010x} rsrc2={rsrc2:#010x} rsrc3={rsrc3:#010x} props={props:#06x} dyn_stack={dyn_stack}"


def main(defines):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    flags = [f for f in HIPCC_FLAGS if f != "-shared"] + defines + ["--cuda-device-only", "--no-gpu-bundle-output", "-c"]
    with tempfile.TemporaryDirectory() as tmp:
        def one(src):
            out = os.path.join(tmp, src + ".co")
            subprocess.run([hipcc] + flags + [os.path.join(CSRC, src), "-o", out], check=True)
            return list(kernels(out))
        with ThreadPoolExecutor(max_workers=8) as ex:
            found = [k for ks in ex.map(one, [s for s in SOURCES if s.endswith(".hip")]) for k in ks]
    names = subprocess.run(["c++filt", "-p"], input="\n".join(k[0] for k in found), capture_output=True, text=True, check=True).stdout.splitlines()
    for name, (_, text, desc) in sorted(zip(names, found)):
        print(f"{name}  sha256={hashlib.sha256(text).hexdigest()}  bytes={len(text)}  {desc}")


if __name__ == "__main__":
    main(sys.argv[1:])
