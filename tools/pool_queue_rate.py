#!/usr/bin/env python3
"""A stream of EXECUTED MACHINES (register rows + program words: what prove_brainfuck(&Machine) receives, mod.rs:471-473) proved on one GPU
from one caller thread, two ways, k proofs in flight:

  (a) batches   the only way before the queue existed: bfhip_trace_create_from_registers for the machines of a batch on the pool's
                sub-contexts — between batches, while the GPU proves nothing —, then bfhip_prove_batch, which returns when the LAST proof
                of the batch is done. The stream is cut into batches of --batch machines; trace creation and the batch boundaries count.
  (b) queue     bfhip_pool_submit_registers with a consumer taking results as they complete; at most --batch jobs outstanding, one more
                submitted for every result taken (the same number of machines in the pool's hands as a batch holds).

  python3 tools/pool_queue_rate.py 22 fib19 --in-flight 3 --batch 12 --machines 24 --rounds 5 --out profiles/pool_queue_rate.txt

(a) and (b) run alternately in ONE process, --rounds times each. Per case and round: ms per proof end to end (wall time of the stream /
machines) and the latency from handing a machine over to holding its proof — (a): from the start of its batch (its trace creation) to the
return of the batch call, (b): from its submit to the wait that returned it — as p50 and max. Every proof's SHA-256 must be the same.
The table goes to stdout and, with --out, to a file; one JSON line per workload follows it."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_batches(pkg, pool, k, rows, words, lmr, n, batch):
    lat, shas = [], set()
    t0 = time.perf_counter()
    for lo in range(0, n, batch):
        m = min(batch, n - lo)
        t_in = time.perf_counter()
        traces = [pkg.Trace.from_registers(pool.ctx(i % k), rows, words) for i in range(m)]
        proofs, _ = pool.prove_batch(traces, lmr)
        t_out = time.perf_counter()
        for t in traces:
            t.close()
        lat += [t_out - t_in] * m
        shas |= {hashlib.sha256(p).hexdigest() for p in proofs}
    return time.perf_counter() - t0, lat, shas


def run_queue(pkg, pool, rows, words, lmr, n, window):
    lat, shas, t_sub = [], set(), {}
    t0 = time.perf_counter()
    sent = 0
    while sent < min(window, n):
        t_sub[pool.submit_registers(rows, words, lmr, tag=sent)] = time.perf_counter(); sent += 1
    for _ in range(n):
        r = pool.wait(600.0)
        now = time.perf_counter()
        if r is None or not r.ok:
            raise SystemExit(f"queue: {r}")
        lat.append(now - t_sub.pop(r.ticket))
        shas.add(hashlib.sha256(r.proof).hexdigest())
        if sent < n:
            t_sub[pool.submit_registers(rows, words, lmr, tag=sent)] = time.perf_counter(); sent += 1
    return time.perf_counter() - t0, lat, shas


def workload(pkg, bench, what, k, batch, n, rounds, mode):
    if what == "fib19":
        code, lmr, name = bench.FIB19, 24, "fib19.bf"
    else:
        code, lmr, name = bench.sweep_program(int(what)), int(what), f"synthetic 2^{int(what)} domain rows"
    _, rows = pkg.host_run(code, b"")
    words = pkg.host_compile(code)
    pool = pkg.Pool(0, n_in_flight=k, max_log_domain=lmr + 2, preprocessed=mode)
    res = {"workload": name, "log_max_rows": lmr, "register_rows": int(rows.shape[0]), "in_flight": k, "batch": batch, "machines": n, "preprocessed_mode": mode,
           "batches": [], "queue": []}
    try:
        run_batches(pkg, pool, k, rows, words, lmr, min(n, batch), batch)          # warm-up of both paths (arena chunks, code objects)
        run_queue(pkg, pool, rows, words, lmr, min(n, batch), batch)
        shas = set()
        for _ in range(rounds):
            for key, fn in (("batches", lambda: run_batches(pkg, pool, k, rows, words, lmr, n, batch)), ("queue", lambda: run_queue(pkg, pool, rows, words, lmr, n, batch))):
                dt, lat, s = fn()
                shas |= s
                res[key].append({"ms_per_proof": round(1e3 * dt / n, 3), "latency_p50_ms": round(1e3 * statistics.median(lat), 2), "latency_max_ms": round(1e3 * max(lat), 2)})
        res["one_proof_sha256"] = len(shas) == 1
    finally:
        pool.close()
    return res


def table(res):
    lines = [f"{res['workload']}  LOG_MAX_ROWS {res['log_max_rows']}, {res['register_rows']} register rows, {res['in_flight']} in flight, "
             f"{res['machines']} machines per round in batches / a window of {res['batch']}, preprocessed mode {res['preprocessed_mode']}",
             "  round  (a) batches: ms/proof  latency p50  max      (b) queue: ms/proof  latency p50  max"]
    for i, (a, b) in enumerate(zip(res["batches"], res["queue"])):
        lines.append(f"  {i + 1:>5}  {a['ms_per_proof']:>21.3f}  {a['latency_p50_ms']:>11.2f}  {a['latency_max_ms']:>7.2f}  {b['ms_per_proof']:>20.3f}  {b['latency_p50_ms']:>11.2f}  {b['latency_max_ms']:>7.2f}")
    ma, mb = [r["ms_per_proof"] for r in res["batches"]], [r["ms_per_proof"] for r in res["queue"]]
    lines.append(f"  median ms/proof: (a) {statistics.median(ma):.3f} (spread {min(ma):.3f}..{max(ma):.3f})   (b) {statistics.median(mb):.3f} (spread {min(mb):.3f}..{max(mb):.3f})"
                 f"   (a) - (b) = {statistics.median(ma) - statistics.median(mb):+.3f} ms; every proof the same SHA-256: {res['one_proof_sha256']}")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", nargs="+", help="fib19, or k for bench.py's synthetic program with 2^k domain rows")
    ap.add_argument("--in-flight", type=int, default=3)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--machines", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--preprocessed", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    import bench
    pkg = bench.load_package()
    lines, results = [], []
    for what in a.what:
        res = workload(pkg, bench, what, a.in_flight, a.batch, a.machines, a.rounds, a.preprocessed)
        results.append(res)
        lines += table(res) + [""]
    text = "\n".join(lines + [json.dumps(r) for r in results]) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
