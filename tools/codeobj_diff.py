#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 code of two builds: python tools/codeobj_diff.py <a> <b>

a, b: object files (the device code is unbundled with llvm-objdump --offloading) or extracted code objects. Prints
the symbols only one side has, the functions whose disassembly differs and the kernels whose resource metadata
differs; exit status 1 on any of them. The order of kernels in the code object is not compared. No GPU needed."""
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
META = ("vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size", "group_segment_fixed_size")


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def code_object(path, tmp):
    with open(path, "rb") as f:
        f.seek(18)   # e_machine: 224 = EM_AMDGPU, already a code object
        if int.from_bytes(f.read(2), "little") == 224:
            return path
    dst = shutil.copy(path, tmp)   # --offloading writes the bundles beside its input
    run("llvm-objdump", "--offloading", dst)
    (co,) = glob.glob(dst + ".*gfx950*")
    return co


def load(path, tmp):
    co = code_object(path, tmp)
    code, name, h = {}, None, None
    for line in run("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^<(.+)>:$", line)
        if m:
            name, h = m.group(1), hashlib.sha256()
            code[name] = h
        elif h is not None:
            text = line.split("//")[0].strip()
            if text and text != "...":   # (a run of zero padding before the next function, which depends on the order)
                h.update(text.encode() + b"\n")
    meta, k = {}, {}
    for line in run("llvm-readelf", "--notes", co).splitlines():
        m = re.match(r"^(  - |    )\.(\w+):\s+(\S+)$", line)   # the keys of an amdhsa.kernels entry, not of its args
        if not m:
            continue
        if m.group(1) == "  - ":
            k = {}
        if m.group(2) in META:
            k[m.group(2)] = m.group(3)
        if m.group(2) == "symbol":   # <kernel>.kd
            meta[m.group(3).removesuffix(".kd")] = k
    return {n: h.hexdigest() for n, h in code.items()}, meta


def main():
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        (ca, ma), (cb, mb) = load(sys.argv[1], ta), load(sys.argv[2], tb)
    bad = 0
    for tag, x, y in (("only in a", ca, cb), ("only in b", cb, ca), ("kernel only in a", ma, mb),
                      ("kernel only in b", mb, ma)):
        for n in sorted(set(x) - set(y)):
            print(f"{tag}: {n}")
            bad += 1
    for n in sorted(set(ca) & set(cb)):
        if ca[n] != cb[n]:
            print(f"code differs: {n}")
            bad += 1
    for n in sorted(set(ma) & set(mb)):
        if ma[n] != mb[n]:
            print(f"metadata differs: {n}: {ma[n]} -> {mb[n]}")
            bad += 1
    print(f"{len(ca)} / {len(cb)} functions, {len(ma)} / {len(mb)} kernels, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
