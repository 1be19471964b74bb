#!/usr/bin/env python3
"""ms per proof under non-default PcsConfigs (include/bfhip.h `bfhip_pcs_config`) and the proof-of-work search on its own.

  python3 tools/pcs_rate.py                      every workload x every config, then the grind timings
  options: --workloads 20,22,fib19 --steps 5 --warmup 2 --grind-only --no-grind --grind-reps 5

One JSON line per run. A proof run: workload, config, security bits, ms per proof = median of `steps` host-clock timings (each call returns
after the proof's last bytes arrived; the context is synchronised before the clock starts) after `warmup` proofs, the 10 phase times of the
median proof, and the host verifier's verdict under the same config. A grind run: bfhip_grind's median time at pow 16, 20, 24, 26 over
`grind-reps` digests (the whole search: every window's launch and read-back). Run the grind part against another build of the library with
BFHIP_LIBRARY=/path/to/libbfhip.so for an A/B. Configs the device prover refuses print their error instead of a time."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

# (name, pow_bits, log_blowup_factor, n_queries): the default, then ~90-bit configs at blowup 1..4
CONFIGS = [("default", 5, 1, 3), ("b1_q70_pow20", 20, 1, 70), ("b2_q35_pow20", 20, 2, 35), ("b3_q24_pow20", 20, 3, 24), ("b4_q18_pow20", 20, 4, 18),
           ("b1_q70_pow24", 24, 1, 70), ("b1_q70_pow26", 26, 1, 70)]


def workload(what):
    if what == "fib19":
        return bench.FIB19, 24, "fib19.bf"
    k = int(what)
    return bench.sweep_program(k), k, f"synthetic 2^{k} domain rows"


def run_proofs(pkg, what, steps, warmup):
    code, lmr, name = workload(what)
    c = pkg.Context(0, max_log_domain=lmr + max(b for _, _, b, _ in CONFIGS) + 1)
    try:
        tr = pkg.Trace(c, code, b"")
        try:
            for cname, pw, b, q in CONFIGS:
                cfg = pkg.PcsConfig(pow_bits=pw, log_blowup_factor=b, n_queries=q)
                line = {"workload": name, "log_max_rows": lmr, "config": cname, **cfg.as_dict(), "security_bits": pkg.security_bits(cfg)}
                try:
                    c.set_pcs_config(cfg)
                except pkg.BfhipError as e:
                    print(json.dumps({**line, "error": str(e)}), flush=True)
                    continue
                for _ in range(warmup):
                    tr.prove(lmr)
                c.sync()
                runs = []
                for _ in range(steps):
                    t0 = time.perf_counter()
                    proof, phases = tr.prove(lmr)
                    runs.append((time.perf_counter() - t0, phases, proof))
                runs.sort(key=lambda r: r[0])
                dt, phases, proof = runs[len(runs) // 2]
                ok, why = pkg.verify_brainfuck(proof, lmr, pcs_config=cfg)
                print(json.dumps({**line, "steps": steps, "ms_per_proof": round(1e3 * dt, 3), "ms_min": round(1e3 * runs[0][0], 3),
                                  "phase_ms": {k: round(v * 1e3, 3) for k, v in phases.items()}, "proof_bytes": len(proof),
                                  "proof_sha256": hashlib.sha256(proof).hexdigest(), "verified": bool(ok), "why": why}), flush=True)
            c.set_pcs_config(None)
        finally:
            tr.close()
    finally:
        c.close()


def run_grind(pkg, reps):
    c = pkg.Context(0, max_log_domain=22)
    try:
        c.grind(hashlib.blake2s(b"warm-up").digest(), 16)
        for pow_bits in (16, 20, 24, 26):
            times, nonces = [], []
            for i in range(reps):
                d = hashlib.blake2s(b"pcs_rate grind %d %d" % (pow_bits, i)).digest()
                c.sync()
                t0 = time.perf_counter()
                nonces.append(c.grind(d, pow_bits))
                times.append(time.perf_counter() - t0)
            print(json.dumps({"grind_pow_bits": pow_bits, "reps": reps, "ms_median": round(1e3 * statistics.median(times), 3),
                              "ms_min": round(1e3 * min(times), 3), "ms_max": round(1e3 * max(times), 3), "nonces": nonces,
                              "ms": [round(1e3 * t, 3) for t in times],
                              "library": os.path.basename(pkg._LIB_PATH)}), flush=True)
    finally:
        c.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="20,22,fib19")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grind-reps", type=int, default=15)
    ap.add_argument("--grind-only", action="store_true")
    ap.add_argument("--no-grind", action="store_true")
    a = ap.parse_args()
    pkg = bench.load_package()
    if not a.grind_only:
        for what in a.workloads.split(","):
            run_proofs(pkg, what, a.steps, a.warmup)
    if not a.no_grind:
        run_grind(pkg, a.grind_reps)


if __name__ == "__main__":
    main()
