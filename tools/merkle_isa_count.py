#!/usr/bin/env python3
"""Instruction census of the Blake2s Merkle layer kernel: compiles stwo-brainfuck_amd/csrc/merkle.hip for gfx950 to assembly (device side only, with
the Makefile's flags) and prints, per k_merkle_layer instantiation and for k_clock_probe, the VALU instructions, the rotations (v_alignbit_b32;
a Blake2s compression has 320, so rotations / 320 = compression sites), the VGPRs and the VALU instructions per compression site.

VALU per site = (VALU - bookkeeping - moves) / sites. "Bookkeeping" is every VALU instruction that cannot belong to a compression: opcodes a
compression does not contain (shifts, 64-bit address arithmetic, compares, selects, and/or/min, multiplies: BOOKKEEPING below) and 32-bit adds with
a scalar-register operand (a compression adds state words, message words and literals, all of them in VGPRs or inline; grid stride and range
offset are kernel arguments in SGPRs). Moves are the register copies of the prefetching loops and of zero words. What remains is adds, xors and
rotations. All three groups are printed, so nothing is hidden in the subtraction. On the general compression (runtime state, counter, flag and 16
message words) this gives the 977 of tools/benchlib (VALU_OPS_PER_COMPRESSION): 320 rotations, 320 + 16 + 2 xors, 320 adds of which half are
three-input. k_clock_probe reads a little higher because its loop also perturbs the message. Constant folding can remove rotations as
well, so sites = rotations / 320 rounded to the nearest integer.

Needs only hipcc (cross-compiles without a GPU).   Usage: python3 tools/merkle_isa_count.py [--src merkle.hip] [-o FILE]"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stwo-brainfuck_amd", "csrc")
ROTATIONS_PER_COMPRESSION = 320      # 10 rounds x 8 G x 4 rotations
KERNELS = ("k_merkle_layer", "k_clock_probe")

# VALU opcodes that only index, address, compare or select: never part of a Blake2s compression
ADD = re.compile(r"^v_add3?_u32")
SGPR = re.compile(r"^s\d+,?$|^s\[")
BOOKKEEPING = re.compile(r"^v_(lshlrev|lshrrev|ashrrev|lshl_add|add_lshl|lshl_or|add_co|addc_co|sub|subrev|mad|mul|cmp|cmpx|cndmask|and|or|min|max|bfe|readfirstlane|readlane)_")


def makefile_flags():
    """CXXFLAGS of the csrc Makefile with $(ARCH) substituted."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= *(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS \?= *(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def compile_asm(src=None, hipcc="hipcc"):
    """Device-side gfx950 assembly of merkle.hip as a list of lines."""
    src = src or os.path.join(CSRC, "merkle.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "merkle.s")
        subprocess.run([hipcc] + makefile_flags() + ["--cuda-device-only", "-S", "-I", CSRC, src, "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


def demangle(names):
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool] + names, capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def count(lines=None):
    """{pretty kernel name: dict(valu, rotations, sites, bookkeeping, vgprs, valu_per_site)} for every kernel in KERNELS."""
    L = lines if lines is not None else compile_asm()
    starts = [(i, l.split(":")[0]) for i, l in enumerate(L) if re.match(r"^_Z\w+:", l)]
    names = demangle([n for _, n in starts])
    res = collections.OrderedDict()
    for (a, name), (b, _) in zip(starts, starts[1:] + [(len(L), "")]):
        pretty = names.get(name, name).split("(")[0].replace("void ", "").replace("bf::", "")
        if not any(k in pretty for k in KERNELS):
            continue
        end = next((i for i in range(a, b) if L[i].startswith(".Lfunc_end")), b)
        ins = [l.split(";")[0].split() for l in L[a:end] if l.startswith("\t") and l.strip() and not l.strip().startswith((".", ";"))]
        valu = [t for t in ins if t[0].startswith("v_")]
        rot = sum(1 for t in valu if t[0].startswith("v_alignbit_b32"))
        moves = sum(1 for t in valu if t[0].startswith("v_mov_b32"))
        book = sum(1 for t in valu if BOOKKEEPING.match(t[0]) or (ADD.match(t[0]) and any(SGPR.match(x) for x in t[2:])))
        vg = next((int(m.group(1)) for l in L[a:b] for m in [re.search(r"; NumVgprs: (\d+)", l)] if m), None)
        sites = int(round(rot / ROTATIONS_PER_COMPRESSION))
        res[pretty] = dict(valu=len(valu), rotations=rot, sites=sites, bookkeeping=book, moves=moves, vgprs=vg,
                           valu_per_site=(len(valu) - book - moves) / sites if sites else float("nan"))
    return res


def report(res):
    out = [f"{'kernel':30s} {'VALU':>6s} {'v_alignbit':>10s} {'sites':>6s} {'bookkeeping':>11s} {'moves':>6s} {'VGPRs':>6s} {'VALU/site':>10s}"]
    for k, r in res.items():
        out.append(f"{k:30s} {r['valu']:6d} {r['rotations']:10d} {r['sites']:6d} {r['bookkeeping']:11d} {r['moves']:6d} {r['vgprs']:6d} {r['valu_per_site']:10.1f}")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    args = sys.argv[1:]
    src = args[args.index("--src") + 1] if "--src" in args else None
    text = report(count(compile_asm(src)))
    sys.stdout.write(text)
    if "-o" in args:
        open(args[args.index("-o") + 1], "w").write(text)
