#!/usr/bin/env python3
"""What the commitment-scheme session (bfhip_pcs_*) costs beside the frozen path on the same trace: fib19 (LOG_MAX_ROWS 24) and the
synthetic 2^22-row trace of tools/benchlib/workloads.py (LOG_MAX_ROWS 22), both runs in ONE process on one box (boxes differ by up to 12 %).

  session  the polynomials of the trace's four trees, captured from one proof (bfhip_test_capture_polys: needs libbfhip_testhooks.so) and
           uploaded once as full-size coefficient columns, pushed through a session with the Brainfuck masks: wall time of the four
           bfhip_pcs_commit calls (form 1) plus bfhip_pcs_prove_values, median of 5 after 2 warm-ups. The bytes are checked against the
           proof's "proof" member every time.
  proof    bfhip_prove_trace of the same resident trace, alternating with the session: the sum of the phases it reports (preprocessed,
           main_trace, interaction, composition, oods, quotients, fri, decommit) minus its logUp generation and its constraint sweep, which
           a session's caller does itself. Those two are priced by HIP events in separate calls (the profiler serialises a proof): the four
           logUp launches as bfhip_trace_check times them on the same trace, k_constraints from one profiled proof.

The session keeps full-size columns where the prover keeps row-granular ones (all of the main trace and the earlier logUp columns: 16x the
words through LDE, leaf hashing, sampling and quotients), reads every root back at once and has no mailbox order.
Output: one block of text per workload (--out FILE also writes it to a file)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("BFHIP_LIBRARY", os.path.join(ROOT, "stwo-brainfuck_amd", "libbfhip_testhooks.so"))
from tools.benchlib.workloads import FIB19, sweep_program                 # noqa: E402
from ratelib import emit, load_package, repeated, require_gpu            # noqa: E402  (first: it puts tests/ on the path)
import pcs_replay                                                         # noqa: E402

PCS_PHASES = ("preprocessed", "main_trace", "interaction", "composition", "oods", "quotients", "fri", "decommit")


def capture(pkg, ctx, tr, log_max_rows):
    """(proof bytes, parsed proof, per-tree log sizes, per-tree device pointers of the captured coefficient columns)"""
    L = pkg.lib()
    assert L.bfhip_test_capture_polys(ctx._h, 1) == 0, L.bfhip_last_error()
    raw, _ = tr.prove(log_max_rows)
    full = json.loads(raw)
    logs = pcs_replay.tree_log_sizes(pkg, tr.log_sizes, log_max_rows)
    ptrs = []
    for t in range(4):
        ptrs.append([])
        for c, log in enumerate(logs[t]):
            out, got = np.empty(1 << log, dtype=np.uint32), ctypes.c_uint32()
            assert L.bfhip_test_captured_poly(ctx._h, t, c, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.size), ctypes.byref(got)) == 0
            assert got.value == log
            ptrs[t].append(ctx.upload(out))
    assert L.bfhip_test_capture_polys(ctx._h, 0) == 0
    return raw, full, logs, ptrs


def session(pkg, ctx, full, logs, ptrs, log_sizes, log_max_rows):
    """One pass of the protocol through a session; returns (seconds in commit x 4 + prove_values, proof bytes)."""
    claimed = [pcs_replay.flat_q(full["interaction_claim"][n]["claimed_sum"]) for n in pcs_replay.NAMES]
    ch = pkg.Channel((0, 0, 0, 0))
    spent = 0.0

    def timed(f, *a, **kw):
        nonlocal spent
        t0 = time.perf_counter()
        r = f(*a, **kw)
        spent += time.perf_counter() - t0
        return r

    with pkg.PcsSession(ctx) as s:
        timed(s.commit, ch, ptrs[0], logs[0], form=1)
        for l in log_sizes:
            ch.mix_u64(l)
        timed(s.commit, ch, ptrs[1], logs[1], form=1)
        for _ in range(3):
            ch.draw_felts(2)
        for c in claimed:
            ch.mix_felts([c])
        timed(s.commit, ch, ptrs[2], logs[2], form=1)
        ch.draw_felts(1)
        timed(s.commit, ch, ptrs[3], logs[3], form=1)
        points, samples = pcs_replay.mask_of(pkg, log_sizes, log_max_rows, ch.draw_point(), 0)
        proof = timed(s.prove_values, ch, points, samples)
    ch.close()
    return spent, proof


def measure(pkg, name, code, log_max_rows, reps, warmup):
    ctx = pkg.Context(0, max_log_domain=log_max_rows + 2)
    tr = pkg.Trace(ctx, code)
    raw, full, logs, ptrs = capture(pkg, ctx, tr, log_max_rows)
    want = pcs_replay.proof_member(raw)
    # the caller's share of a proof, by HIP events: logUp generation (as bfhip_trace_check times the same four launches) and k_constraints
    def check_then_prove():
        assert tr.check().ok
        tr.prove(log_max_rows, want_json=False)

    priced = [ms for _, ms in repeated(ctx, check_then_prove, 3, 0)]
    logup_ms, sweep_ms = statistics.median(ms["trace_check_logup"] for ms in priced), statistics.median(ms["k_constraints"] for ms in priced)
    ses, prf, tot = [], [], []
    for i in range(warmup + reps):
        dt, proof = session(pkg, ctx, full, logs, ptrs, tr.log_sizes, log_max_rows)
        assert proof == want, "the session's bytes differ from the proof's"
        _, ph = tr.prove(log_max_rows, want_json=False)
        if i >= warmup:
            ses.append(1e3 * dt); prf.append(1e3 * sum(ph[k] for k in PCS_PHASES)); tot.append(1e3 * ph["total"])
    words = sum(1 << l for t in logs for l in t)
    for t in ptrs:
        for p in t:
            ctx.free(p)
    tr.close(); ctx.close()
    med = statistics.median
    s, p = med(ses), med(prf) - logup_ms - sweep_ms
    return [f"{name}: LOG_MAX_ROWS {log_max_rows}, component log sizes {tr.log_sizes}, {sum(len(t) for t in logs)} columns, {words * 4 / 2**20:.0f} MiB of full-size coefficients",
            f"  session: 4 x commit + prove_values, wall     median {s:.3f} ms of {reps} (min {min(ses):.3f}, max {max(ses):.3f})",
            f"  proof: sum of its phases                     median {med(prf):.3f} ms (min {min(prf):.3f}, max {max(prf):.3f}); total {med(tot):.3f} ms",
            f"  proof: logUp generation / constraint sweep   {logup_ms:.3f} ms / {sweep_ms:.3f} ms by HIP events (median of 3)",
            f"  proof without those two                      {p:.3f} ms",
            f"  session / proof without those two            {s / p:.3f}"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--out")
    ap.add_argument("--only", choices=("fib19", "2p22"))
    a = ap.parse_args()
    pkg = load_package()
    require_gpu(pkg, "pcs_session_rate")
    lines = []
    for key, name, code, lmr in (("fib19", "fib19", FIB19, 24), ("2p22", "synthetic 2^22 rows", sweep_program(22), 22)):
        if a.only in (None, key):
            lines += measure(pkg, name, code, lmr, a.reps, a.warmup) + [""]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    emit("\n".join(lines) + "\n", a.out)


if __name__ == "__main__":
    main()
