#!/usr/bin/env python3
"""bfhip_grind_poseidon252 (the Poseidon252Channel proof-of-work search) beside its yardstick, in one run on one GPU.

  python3 tools/grind_poseidon_rate.py [--reps 15] [--warmup 2] [--pows 12,16,20,24,28] [--ubench PATH] [--out profiles/grind_poseidon_rate.txt]

  search     per pow_bits: `reps` fixed digests (sha256("grind_poseidon_rate <pow_bits> <i>") mod p) after `warmup` calls on other digests.
             ms per call = host clock around the whole call (every span's launch and read-back; the context is synchronised before the
             clock starts): median and range. Permutations per second = nonces scanned (`tried`, launches x span) / GPU time of the
             launches by HIP events (Context.profiling, one event pair per launch), summed over the `reps` calls.
  yardstick  Hades permutations per second with the state in registers: `k_hades` of tools/ubench_poseidon.hip, the same field code with no
             conversion, no test and no read-back. The program is run 5 times before the search and 5 times after it (median and range).
             --ubench names a built binary; without it the source is compiled with hipcc into a temporary directory.
  CPU        the CPU oracle's orc_grind_digest under the Poseidon252 channel on the first 3 digests at pow_bits 16 and 20.

A run without a GPU fails: nothing here is measured on the host except the CPU oracle's own time."""
import argparse
import ctypes
import hashlib
import os
import re
import statistics
import subprocess
import tempfile
import time

from ratelib import ROOT, Oracle, cell, emit, load_package, require_gpu

P252 = 2**251 + 17 * 2**192 + 1


def digest(pow_bits, i):
    return (int.from_bytes(hashlib.sha256(b"grind_poseidon_rate %d %d" % (pow_bits, i)).digest(), "big") % P252).to_bytes(32, "little")


def yardstick(binary, runs=5):
    rates = []
    for _ in range(runs):
        out = subprocess.run([binary], capture_output=True, text=True, timeout=120, check=True).stdout
        rates.append(1e6 * float(re.search(r"Hades permutations \(registers only\): ([0-9.]+) M/s", out).group(1)))
    return rates


def search(pkg, ctx, pow_bits, reps, warmup):
    for i in range(warmup):
        ctx.grind_poseidon252(digest(pow_bits, 1000 + i), pow_bits)
    ms, nonces, tried_all = [], [], 0
    with ctx.profiling(1):      # every call is another digest and is timed on its own; one report over the `reps` calls
        for i in range(reps):
            d = digest(pow_bits, i)
            ctx.sync()
            t0 = time.perf_counter()
            nonce, tried = ctx.grind_poseidon252(d, pow_bits, with_tried=True)
            ms.append(1e3 * (time.perf_counter() - t0))
            nonces.append(nonce); tried_all += tried
        rec = ctx.profile_report()["k_grind_poseidon"]
    assert rec["units"] == tried_all, (rec, tried_all)
    return {"pow_bits": pow_bits, "ms": ms, "nonces": nonces, "tried": tried_all, "launches": rec["calls"], "gpu_ms": rec["total_ms"],
            "perm_per_s": tried_all / (rec["total_ms"] * 1e-3)}


def cpu_oracle(pow_bits, n=3):
    orc = Oracle()
    orc.L.orc_grind_digest.restype = ctypes.c_uint64
    orc.set_conventions(0, 0, 0, 1)
    try:
        out = []
        for i in range(n):
            t0 = time.perf_counter()
            nonce = orc.L.orc_grind_digest(digest(pow_bits, i), ctypes.c_uint32(pow_bits))
            out.append((nonce, 1e3 * (time.perf_counter() - t0)))
        return out
    finally:
        orc.set_conventions(0, 0, 0, 0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pows", default="12,16,20,24,28"); ap.add_argument("--ubench"); ap.add_argument("--out")
    a = ap.parse_args()
    pkg = load_package()
    require_gpu(pkg, "grind_poseidon_rate")
    tmp = None
    binary = a.ubench
    if not binary:
        tmp = tempfile.TemporaryDirectory()
        binary = os.path.join(tmp.name, "ubench_poseidon")
        subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "stwo-brainfuck_amd", "csrc"), "-o", binary,
                        os.path.join(ROOT, "tools", "ubench_poseidon.hip")], check=True)
    pows = [int(p) for p in a.pows.split(",")]
    before = yardstick(binary)
    ctx = pkg.Context(0, max_log_domain=16)
    try:
        rows = [search(pkg, ctx, pw, a.reps, a.warmup) for pw in pows]
    finally:
        ctx.close()
    after = yardstick(binary)
    yard = statistics.median(before + after)
    lines = [f"bfhip_grind_poseidon252: {a.reps} digests per pow_bits after {a.warmup} warm-ups; span per launch 2^clamp(pow_bits - 4, 12, 20)",
             f"yardstick k_hades (tools/ubench_poseidon.hip, registers only), permutations/s: median {yard:.4g} of {len(before + after)} runs "
             f"(before the search {min(before):.4g}-{max(before):.4g}, after it {min(after):.4g}-{max(after):.4g})", "",
             "pow_bits | ms per call: median (min-max) | launches | nonces scanned | GPU ms by HIP events | permutations/s | of the yardstick"]
    for r in rows:
        lines.append(f"{r['pow_bits']:8d} | {cell(r['ms'], 3)} | {r['launches']} | {r['tried']} | "
                     f"{r['gpu_ms']:.3f} | {r['perm_per_s']:.4g} | {r['perm_per_s'] / yard:.3f}")
    lines.append("")
    for r in rows:
        lines.append(f"pow_bits {r['pow_bits']}: nonces {r['nonces']}")
        lines.append(f"pow_bits {r['pow_bits']}: ms {[round(m, 3) for m in r['ms']]}")
    lines.append("")
    for pw in (16, 20):
        res = cpu_oracle(pw)
        lines.append(f"CPU oracle orc_grind_digest, pow_bits {pw}: " + ", ".join(f"nonce {n} in {ms:.1f} ms" for n, ms in res)
                     + f"  ({1e3 * sum(n + 1 for n, _ in res) / sum(ms for _, ms in res):.4g} permutations/s, one thread)")
    emit("\n".join(lines) + "\n", a.out)
    if tmp:
        tmp.cleanup()


if __name__ == "__main__":
    main()
