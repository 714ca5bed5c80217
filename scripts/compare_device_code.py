#!/usr/bin/env python3
"""Is the device code of two builds of the library the same?  For refactors of the kernel headers that must not change a kernel.

usage: compare_device_code.py <csrc before> <csrc after> [object directory | object.o ...]      (default: build build_df)

Both trees have been built (`make` and `make check-forms-lib` in juqbox.jl_amd/csrc).  For every <tag>.flags of an object directory
the gfx950 code object is taken out of <tag>.o of either tree and three things are compared:
  text    llvm-objdump -d of the code object (every instruction of every kernel; the lines that hold the file name are skipped)
  rodata  llvm-objdump -s -j .rodata (the kernel descriptors: registers, scratch, LDS, ...)
  usage   the per-kernel remarks of <tag>.log (registers, spills, scratch, LDS, occupancy) without their source locations
plus the flags themselves, and per object directory manifest.json (keys that hold a hash aside).  The whole ELF is no use: two compiles
of one source differ in a per-compile identifier of the symbol tables.  An argument that ends in .o names a single object of both trees
that has no .flags / .log (build/host.o: the auxiliary kernels): text and rodata only.  Prints one row per object -- the SHA-256 prefix over text and
rodata before and after -- and exits 1 unless everything is equal."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def device_dumps(obj, tmp):
    """(disassembly, .rodata dump) of the gfx950 code object inside a host object compiled by hipcc"""
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, "unused.o"))
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co)
    dumps = []
    for args in (("-d",), ("-s", "-j", ".rodata")):
        out = run(os.path.join(LLVM, "llvm-objdump"), *args, co)
        dumps.append("\n".join(ln for ln in out.splitlines() if "file format" not in ln))
    return dumps


def usage_lines(log):
    """the resource-usage remarks of a compile log, source locations stripped"""
    # ("file:line:col: remark: text" -- with -save-temps "remark: file:line:col: text")
    return [m.group(1).strip() for m in (re.search(r"remark: (?:\S+:\d+:\d+: )?(.*) \[-Rpass-analysis=kernel-resource-usage\]", ln)
                                         for ln in open(log, errors="replace")) if m]


def without_hashes(x):
    if isinstance(x, dict):
        return {k: without_hashes(v) for k, v in x.items() if "hash" not in k.lower()}
    return [without_hashes(v) for v in x] if isinstance(x, list) else x


def sha(*parts):
    return hashlib.sha256("\0".join(parts).encode()).hexdigest()[:16]


def main():
    before, after = sys.argv[1:3]
    dirs = sys.argv[3:] or ["build", "build_df"]
    bad = 0
    print("# object  sha256(text + rodata) before  after  verdict")
    with tempfile.TemporaryDirectory() as tmp:
        for d in dirs:
            if d.endswith(".o"):
                dumps = [device_dumps(os.path.join(t, d), tmp) for t in (before, after)]
                diff = [what for i, what in enumerate(("text", "rodata")) if dumps[0][i] != dumps[1][i]]
                print("%s  %s  %s  %s" % (d, sha(*dumps[0]), sha(*dumps[1]), "DIFFERS: " + " ".join(diff) if diff else "same"))
                bad += bool(diff)
                continue
            tags = sorted(f[:-6] for f in os.listdir(os.path.join(before, d)) if f.endswith(".flags"))
            tags_after = sorted(f[:-6] for f in os.listdir(os.path.join(after, d)) if f.endswith(".flags"))
            if tags != tags_after:
                print("%s: the object lists differ: %s" % (d, sorted(set(tags) ^ set(tags_after))))
                bad += 1
            for tag in tags:
                if tag not in tags_after:
                    continue
                diff, h = [], []
                sides = [os.path.join(t, d, tag) for t in (before, after)]
                dumps = [device_dumps(s + ".o", tmp) for s in sides]
                for i, what in enumerate(("text", "rodata")):
                    if dumps[0][i] != dumps[1][i]:
                        diff.append(what)
                if usage_lines(sides[0] + ".log") != usage_lines(sides[1] + ".log"):
                    diff.append("usage")
                if open(sides[0] + ".flags").read() != open(sides[1] + ".flags").read():
                    diff.append("flags")
                h = [sha(*dm) for dm in dumps]
                print("%s/%s  %s  %s  %s" % (d, tag, h[0], h[1], "DIFFERS: " + " ".join(diff) if diff else "same"))
                bad += bool(diff)
            man = [without_hashes(json.load(open(os.path.join(t, d, "manifest.json")))) for t in (before, after)]
            print("%s/manifest.json  %s" % (d, "same" if man[0] == man[1] else "DIFFERS"))
            bad += man[0] != man[1]
            print("# %s: %d objects" % (d, len(tags)))
    print("# %s" % ("every object: same device code, same resource usage, same flags" if not bad else "%d DIFFERENCE(S)" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
