#!/usr/bin/env python3
"""Device code identity of two source trees, kernel by kernel.

    tools/kernel_identity.py <parent tree> <this tree>

Compiles every antidote_ccrdt_amd/csrc/*.hip of each tree to a device-only
code object (a plain ELF) with the Makefile's compiler and CXXFLAGS and
records, per kernel symbol and whichever file it came from: a hash of the
function's bytes in .text, the 64-byte kernel descriptor (.kd) with
kernel_code_entry_byte_offset (bytes 16..23, a matter of layout) zeroed, the
descriptor's size, and the kernel's resource entry of the NT_AMDGPU_METADATA
note.  Prints one line per kernel that differs, is missing or is new, then
"N kernels, D differ"; exits non-zero unless D == 0 and both trees hold the
same kernels.  Bytes are read and hashed, never decoded.  A refactor that only
moves kernels between files must leave every one of them identical."""
import glob
import hashlib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import yaml

CSRC = os.path.join("antidote_ccrdt_amd", "csrc")
META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".kernarg_segment_size", ".max_flat_workgroup_size")


def run(*cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def compile_co(tree, src, out):
    # "<hipcc> <CXXFLAGS>" as the Makefile expands them
    cc = run("make", "-s", "-C", os.path.join(tree, CSRC), "--eval", "print-cc: ; @echo $(HIPCC) $(CXXFLAGS)",
             "print-cc").split()
    run(*cc, "--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", out, cwd=os.path.join(tree, CSRC))
    return out


def kernels_of(co, readelf):
    """{mangled name: (text hash, kd bytes, kd size, metadata)} of one code object."""
    blob = open(co, "rb").read()
    secs = {}  # section index -> (address, file offset)
    for ln in run(readelf, "-SW", co).splitlines():
        f = ln.replace("[", " ").replace("]", " ").split()
        if len(f) > 5 and f[0].isdigit() and f[1].startswith("."):
            secs[int(f[0])] = (int(f[3], 16), int(f[4], 16))
    syms = {}  # name -> bytes
    for ln in run(readelf, "-sW", "--dyn-syms", co).splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            addr, off = secs[int(f[6])]
            at = int(f[1], 16) - addr + off
            syms[f[7]] = blob[at:at + int(f[2])]
    notes = run(readelf, "--notes", co)
    doc = yaml.safe_load(notes[notes.index("---"):notes.rindex("...")])
    out = {}
    for k in doc.get("amdhsa.kernels") or []:
        kd = bytearray(syms[k[".symbol"]])
        kd[16:24] = bytes(8)
        out[k[".name"]] = (hashlib.sha256(syms[k[".name"]]).hexdigest(), bytes(kd), len(kd),
                           tuple(k.get(m) for m in META))
    return out


def kernels_of_tree(tree, tmp, tag):
    tree = os.path.abspath(tree)
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    srcs = sorted(glob.glob(os.path.join(tree, CSRC, "*.hip")))
    with ThreadPoolExecutor(min(16, os.cpu_count() or 8)) as ex:
        cos = list(ex.map(lambda s: compile_co(tree, s, os.path.join(
            tmp, tag + "_" + os.path.basename(s)[:-4] + ".co")), srcs))
    all_k = {}
    for s, co in zip(srcs, cos):
        for name, rec in kernels_of(co, readelf).items():
            if name in all_k:
                raise SystemExit(f"{tree}: kernel {name} defined twice")
            all_k[name] = rec + (os.path.basename(s),)
    return all_k


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        a = kernels_of_tree(sys.argv[1], tmp, "a")
        b = kernels_of_tree(sys.argv[2], tmp, "b")
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in b:
            why = f"missing (was in {a[name][4]})"
        elif name not in a:
            why = f"new (in {b[name][4]})"
        else:
            parts = ("text", "kd", "kd size", "metadata")
            diff = [p for p, x, y in zip(parts, a[name], b[name]) if x != y]
            if not diff:
                continue
            why = f"differs in {', '.join(diff)} ({a[name][4]} -> {b[name][4]})"
            if "metadata" in diff:
                why += f" {dict(zip(META, a[name][3]))} -> {dict(zip(META, b[name][3]))}"
        bad += 1
        print(f"{name}: {why}")
    n = f"{len(a)}" if len(a) == len(b) else f"{len(a)} -> {len(b)}"
    print(f"{n} kernels, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
