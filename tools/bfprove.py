#!/usr/bin/env python3
"""prove | verify over the C ABI — the two sub-commands of the reference's bin/brainfuck_prover.rs (prove: :79-139, verify: :141-151) —, check,
the reference's `assert_constraints` (memory/component.rs:201-208, mod.rs:252-396) for a whole execution, and relations, stwo's relation
tracker for it:

  bfprove.py prove  (--file prog.bf | --code '++>,<[>+.<-]') [--input-file in.bin] [--ram-size N] [--output proof.json]
                    [--log-max-rows 24] [--conventions a,b,c,d | --poseidon252] [--all-sets DIR] [PCS options]
                    [--preflight] [--set-register ROW:NAME=VALUE ...] [--set-word INDEX=VALUE ...] [--generic]
  bfprove.py prove  --queue N --programs a.bf b.bf ... --output-dir DIR [--input-file in.bin] [--ram-size N] [--log-max-rows 24]
                    [--conventions a,b,c,d | --poseidon252] [PCS options] [--preflight] [--set-register ...] [--generic]
  bfprove.py verify proof.json [--log-max-rows 24] [--conventions a,b,c,d | --poseidon252 | --try-all] [PCS options] [--generic]
  bfprove.py check  (--file prog.bf | --code '++>,<[>+.<-]') [--input-file in.bin] [--ram-size N] [--set-register ROW:NAME=VALUE ...]
  bfprove.py relations (--file prog.bf | --code ...) [--input-file in.bin] [--ram-size N] [--set-register ROW:NAME=VALUE ...]
                    [--set-word INDEX=VALUE ...] [--max-entries 64]

check runs the program on the host VM, hands the register trace to the GPU (bfhip_trace_create_from_registers) and asserts the 13 AIRs on
the trace domain (bfhip_trace_check). It prints `ok`, or one line per failing component — e.g.
"memory: constraint 6 fails at table row 0 (cell 0), value (2, 0, 0, 0); 16 cells violate it" — and exits with 1: what lies behind a proof
that fails with ConstraintsNotSatisfied. --set-register alters one register (clk, ip, ci, ni, mp, mv, mvi) of one row of the executed
trace first: what a faulty VM would hand over.

relations builds the same trace and lists the lookup tuples that do not cancel (bfhip_trace_relations): `balanced`, or one line per tuple —
e.g. "processor relation: (1, 1, 35, 43, 0, 1, 1) net +1: yielded 1x (first: processor row 1), used 0x" — and exit code 1: what lies behind
a logUp total that is not zero while every component checks `ok`. --set-word alters one word of the compiled program as well (an opcode
that is no instruction has to appear in the program and in the register rows).

prove --queue N proves a list of programs N at a time through the pool's queue (bfhip_pool_submit_registers / bfhip_pool_wait): every program
is run on the host VM, its executed machine is submitted, and each proof is written to DIR/<program name>.proof.json as it completes — in
completion order, one line per proof on stdout. A program that fails (too large for --log-max-rows, input exhausted) is reported with its
own error and does not stop the others; the exit code is 1 if any failed.

prove --preflight switches on the proof's own filter (bfhip_ctx_set_preflight / bfhip_pool_set_preflight): the 13 AIRs and the logUp total
are asserted on the tables before the proof starts, and a trace that cannot be proved is refused with the lines check and relations would
print — "TraceRejected: 1 of 13 components violate their constraints ..." on stdout, exit code 1 — instead of a proof's worth of GPU time and
"ConstraintsNotSatisfied". In --queue mode a rejected program is reported with those lines and does not stop the others. --set-register /
--set-word hand the prover the executed machine with one register / program word altered (in --queue mode: of every program).

prove --generic proves the same trace through bfhip_air_prove: the 13 components as constraint and fraction programs under
brainfuck_air_statement, the main trace handed over as full-size device columns, IsFirst as coefficients. The file it writes is the same
BrainfuckProof (claim and interaction claim put around the driver's claimed sums and proof member) — byte for byte the file of the
built-in path, which plain `verify` accepts. verify --generic checks a BrainfuckProof file through bfhip_air_verify under the statement
that its claim describes. Neither works with --all-sets or --preflight. prove --generic --queue N --programs ... sends every program's trace
through the pool's queue as an AIR statement (bfhip_pool_submit_air), N in flight, and writes the same files as --queue alone.

PCS options (stwo's PcsConfig; the defaults are PcsConfig::default()): --pow-bits 5 --log-blowup-factor 1 --n-queries 3. The proof file does
not record them: verify with the values the proof was made with. prove prints the config and its security bits (pow + blowup x queries).

The proof file is the serde_json form of BrainfuckProof (mod.rs:71-76), as the reference writes it (:129-131) and reads it (:146-151).
stdin supplies the program input when --input-file is absent (the reference's VM reads stdin).

--conventions merkle_node_hash,mix_u64,logup_mask_order,merkle_channel — the byte-level switches of include/bfhip.h `bfhip_conventions`
(all 0 = the defaults). The two commands below are the one-step pin against the real stwo@31e8dbc for whoever has cargo:

  verify --try-all      a proof written by `brainfuck_prover prove --output` is checked under every switch set (8 Blake2s + 2 Poseidon252);
                        prints the accepting set(s), or for every set the first check that fails. Host only: no GPU needed.
  prove --all-sets DIR  writes this prover's proof of the program under each of the 8 Blake2s switch sets to DIR/proof_<a><b><c>0.json, for
                        `brainfuck_prover verify DIR/proof_*.json`: the file the reference accepts names the conventions of its stwo."""
import argparse
import itertools
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package
import pcs_replay

NAMES = ("merkle_node_hash", "mix_u64", "logup_mask_order", "merkle_channel")
VALUES = (("stwo-compress", "rfc7693"), ("compress", "hash"), ("[0,-1]", "[-1,0]"), ("blake2s", "poseidon252"))


def parse_conventions(a):
    if a.conventions:
        conv = tuple(int(v) for v in a.conventions.split(","))
        if len(conv) != 4 or any(v not in (0, 1) for v in conv):
            raise SystemExit("--conventions takes four 0/1 values: " + ",".join(NAMES))
        return conv
    return (0, 0, 0, 1 if a.poseidon252 else 0)


def describe(conv):
    return ", ".join(f"{n}={VALUES[i][v]}" for i, (n, v) in enumerate(zip(NAMES, conv)))


def all_sets(channels=(0, 1)):
    """The 8 Blake2s switch sets, and for the Poseidon252 channel the 2 that differ there (the node-hash and mix_u64 switches are Blake2s forms)."""
    sets = []
    for d in channels:
        for a, b, c in itertools.product((0, 1), repeat=3):
            if d == 0 or (a, b) == (0, 0):
                sets.append((a, b, c, d))
    return sets


def add_pcs_options(p):
    p.add_argument("--pow-bits", type=int, default=5); p.add_argument("--log-blowup-factor", type=int, default=1)
    p.add_argument("--n-queries", type=int, default=3)


def parse_pcs(pkg, a):
    return pkg.PcsConfig(pow_bits=a.pow_bits, log_blowup_factor=a.log_blowup_factor, n_queries=a.n_queries)


def try_all(pkg, proof, log_max_rows, pcs_config=None):
    """Verifies `proof` under every convention set. Returns (accepting sets, {set: first failing check})."""
    accepted, reasons = [], {}
    for conv in all_sets():
        try:
            ok, why = pkg.verify_brainfuck(proof, log_max_rows, conventions=conv, pcs_config=pcs_config)
        except Exception as e:                      # a proof of the other channel's shape does not even parse
            ok, why = False, f"error: {e}"
        if ok:
            accepted.append(conv)
        else:
            reasons[conv] = why
    return accepted, reasons


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("prove")
    p.add_argument("--file"); p.add_argument("--code"); p.add_argument("--input-file"); p.add_argument("--ram-size", type=int, default=0)
    p.add_argument("--output"); p.add_argument("--log-max-rows", type=int, default=24); p.add_argument("--poseidon252", action="store_true")
    p.add_argument("--conventions"); p.add_argument("--all-sets", metavar="DIR")
    p.add_argument("--queue", type=int, default=0, metavar="N", help="prove --programs through the pool's queue, N proofs in flight")
    p.add_argument("--programs", nargs="+", default=[], metavar="FILE"); p.add_argument("--output-dir", metavar="DIR")
    p.add_argument("--preflight", action="store_true", help="reject a trace that cannot be proved before proving it, naming row and tuple")
    p.add_argument("--set-register", action="append", default=[], metavar="ROW:NAME=VALUE"); p.add_argument("--set-word", action="append", default=[], metavar="INDEX=VALUE")
    p.add_argument("--generic", action="store_true", help="prove through bfhip_air_prove with the 13 components as programs")
    v = sub.add_parser("verify")
    v.add_argument("proof"); v.add_argument("--log-max-rows", type=int, default=24); v.add_argument("--poseidon252", action="store_true")
    v.add_argument("--conventions"); v.add_argument("--try-all", action="store_true")
    v.add_argument("--generic", action="store_true", help="verify through bfhip_air_verify under brainfuck_air_statement")
    k = sub.add_parser("check")
    k.add_argument("--file"); k.add_argument("--code"); k.add_argument("--input-file"); k.add_argument("--ram-size", type=int, default=0)
    k.add_argument("--set-register", action="append", default=[], metavar="ROW:NAME=VALUE")
    r = sub.add_parser("relations")
    r.add_argument("--file"); r.add_argument("--code"); r.add_argument("--input-file"); r.add_argument("--ram-size", type=int, default=0)
    r.add_argument("--set-register", action="append", default=[], metavar="ROW:NAME=VALUE")
    r.add_argument("--set-word", action="append", default=[], metavar="INDEX=VALUE"); r.add_argument("--max-entries", type=int, default=64)
    add_pcs_options(p); add_pcs_options(v)
    a = ap.parse_args()
    pkg = load_package()
    try:
        return run(pkg, a, ap)
    except pkg.BfhipError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2


REGISTERS = ("clk", "ip", "ci", "ni", "mp", "mv", "mvi")


def executed_machine(pkg, a, ap, code, inp):
    """The program run on the host VM, --set-register / --set-word applied: (register rows, program words)."""
    _, rows = pkg.host_run(code, inp, ram_size=a.ram_size)
    for spec in a.set_register:
        try:
            row, rest = spec.split(":")
            name, value = rest.split("=")
            rows[int(row), REGISTERS.index(name)] = int(value)
        except (ValueError, IndexError):
            ap.error(f"--set-register takes ROW:NAME=VALUE with NAME one of {', '.join(REGISTERS)} and ROW < {rows.shape[0]}, got {spec!r}")
    words = pkg.host_compile(code)
    for spec in getattr(a, "set_word", []):
        try:
            index, value = spec.split("=")
            words[int(index)] = int(value)
        except (ValueError, IndexError):
            ap.error(f"--set-word takes INDEX=VALUE with INDEX < {words.size}, got {spec!r}")
    return rows, words


def executed_trace(pkg, a, ap):
    """The executed machine of --file / --code as a resident trace: (context, trace)."""
    code = open(a.file).read() if a.file else a.code
    if code is None:
        ap.error(f"{a.cmd} needs --file or --code")
    inp = open(a.input_file, "rb").read() if a.input_file else (b"" if sys.stdin.isatty() else sys.stdin.buffer.read())
    rows, words = executed_machine(pkg, a, ap, code, inp)
    ctx = pkg.Context(0, max_log_domain=8)       # neither the check nor the relation summary needs a twiddle tree
    return ctx, pkg.Trace.from_registers(ctx, rows, words)


def check(pkg, a, ap):
    ctx, tr = executed_trace(pkg, a, ap)
    res = tr.check()
    tr.close(); ctx.close()
    for line in res.failures():
        print(line)
    if res.ok:
        print("ok")
    return 0 if res.ok else 1


def relations(pkg, a, ap):
    ctx, tr = executed_trace(pkg, a, ap)
    res = tr.relations(a.max_entries)
    tr.close(); ctx.close()
    for line in res.lines():
        print(line)
    if res.balanced:
        print("balanced")
    return 0 if res.balanced else 1


def prove_queue(pkg, a, ap):
    """prove --queue N: the programs' executed machines through bfhip_pool_submit_registers, each proof written as it completes."""
    if not a.programs or not a.output_dir:
        ap.error("prove --queue needs --programs FILE... and --output-dir DIR")
    if not 1 <= a.queue <= 16:
        ap.error("--queue takes 1..16 proofs in flight")
    inp = open(a.input_file, "rb").read() if a.input_file else (b"" if sys.stdin.isatty() else sys.stdin.buffer.read())
    os.makedirs(a.output_dir, exist_ok=True)
    pcs = parse_pcs(pkg, a)
    pool = pkg.Pool(0, n_in_flight=a.queue, max_log_domain=a.log_max_rows + pcs.log_blowup_factor + 1)
    failed = 0
    try:
        pool.set_pcs_config(pcs)
        pool.set_conventions(*parse_conventions(a))
        if a.preflight:
            pool.set_preflight(True)
        t0 = time.time()
        for i, path in enumerate(a.programs):
            code = open(path).read()
            try:
                rows, words = executed_machine(pkg, a, ap, code, inp)
                pool.submit_registers(rows, words, a.log_max_rows, tag=i)
            except pkg.BfhipError as e:            # the VM refused the program: nothing was submitted
                failed += 1
                print(f"{path}: error: {e}", file=sys.stderr)
        for r in pool.as_completed(timeout_s=3600.0):
            path = a.programs[r.tag]
            if r.rejected:                         # --preflight: the rejection lines, "job <ticket>: TraceRejected: ..." first
                failed += 1
                print(f"{path}: {r.error}", flush=True)
                continue
            if not r.ok:
                failed += 1
                print(f"{path}: error: {r.error}", file=sys.stderr)
                continue
            out = os.path.join(a.output_dir, os.path.splitext(os.path.basename(path))[0] + ".proof.json")
            open(out, "wb").write(r.proof)
            print(f"{out}  {len(r.proof)} bytes; queued {1e3 * r.seconds_queued:.1f} ms, proving {1e3 * r.seconds_proving:.1f} ms on worker {r.worker}; "
                  f"{time.time() - t0:.3f}s after the first submit", flush=True)
    finally:
        pool.close()
    return 1 if failed else 0


def generic_columns(pkg, ctx, tr, log_max_rows):
    """The caller trees of brainfuck_air_statement for a resident trace, as device columns: ([IsFirst coefficients of log sizes log_max_rows
    .. 4], [the main trace, components in claim order, every column full size]) and every pointer to free."""
    pre = [ctx.malloc(4 << n) for n in range(4, log_max_rows + 1)]
    ctx.is_first_coeffs(4, log_max_rows, pre)
    main, scratch = [], []
    for k in range(13):
        n = 1 << tr.log_sizes[k]
        for j in range(pkg._BF_N_MAIN[k]):
            rows = tr.column(k, j)
            src = ctx.upload(rows)
            if len(rows) == n:
                main.append(src)
                continue
            assert 16 * len(rows) == n, "a resident trace holds row-granular columns"
            scratch.append(src)
            main.append(ctx.malloc(4 * n))
            ctx.broadcast16(src, main[-1], len(rows))
    ctx.sync()
    for p in scratch:
        ctx.free(p)
    return [pre[::-1], main], pre + main


def generic_prove(pkg, ctx, tr, log_max_rows, conv, kernels=None, columns=None):
    """(the BrainfuckProof bytes, air_prove's own result) of a resident trace through bfhip_air_prove"""
    st = pkg.brainfuck_air_statement(tr.log_sizes, log_max_rows, conv[2])
    cols, ptrs = columns or generic_columns(pkg, ctx, tr, log_max_rows)
    try:
        with pkg.Channel(conv) as ch:
            raw = ctx.air_prove(st, cols, ch, kernels=kernels)
    finally:
        if columns is None:
            for p in ptrs:
                ctx.free(p)
    return brainfuck_proof_of(raw, tr.log_sizes), raw


def brainfuck_proof_of(raw, log_sizes):
    """The BrainfuckProof bytes around air_prove's result: claim and interaction claim put around its claimed sums and proof member"""
    head, at = b'{"claimed_sums":[', raw.index(b'],"proof":')
    sums = raw[len(head): at].replace(b"]],[[", b"]]\n[[").split(b"\n")
    assert raw.startswith(head) and len(sums) == 13
    claim = b",".join(b'"%s":{"log_size":%d,"_marker":null}' % (n.encode(), l) for n, l in zip(pcs_replay.NAMES, log_sizes))
    inter = b",".join(b'"%s":{"claimed_sum":%s}' % (n.encode(), c) for n, c in zip(pcs_replay.NAMES, sums))
    return b'{"claim":{' + claim + b'},"interaction_claim":{' + inter + b'},"proof":' + raw[at + len(b'],"proof":'):]


def prove_queue_generic(pkg, a, ap):
    """prove --generic --queue N: every program's trace as a brainfuck_air_statement job of the pool's queue (bfhip_pool_submit_air), each
    proof written as it completes. The traces are made resident by a context of the caller's; the columns of every program stay on the
    device until its result has been taken."""
    if not a.programs or not a.output_dir:
        ap.error("prove --queue needs --programs FILE... and --output-dir DIR")
    if not 1 <= a.queue <= 16:
        ap.error("--queue takes 1..16 proofs in flight")
    if a.set_register or a.set_word:
        ap.error("--generic --queue does not go with --set-register / --set-word")
    inp = open(a.input_file, "rb").read() if a.input_file else (b"" if sys.stdin.isatty() else sys.stdin.buffer.read())
    os.makedirs(a.output_dir, exist_ok=True)
    pcs, conv = parse_pcs(pkg, a), parse_conventions(a)
    max_log_domain = a.log_max_rows + pcs.log_blowup_factor + 1
    ctx = pkg.Context(0, max_log_domain=max_log_domain)
    pool = pkg.Pool(0, n_in_flight=a.queue, max_log_domain=max_log_domain)
    failed, held = 0, {}
    try:
        pool.set_pcs_config(pcs)
        pool.set_conventions(*conv)
        t0 = time.time()
        with pkg.Channel(conv) as ch:
            for i, path in enumerate(a.programs):
                try:
                    tr = pkg.Trace(ctx, open(path).read(), inp, ram_size=a.ram_size)
                except pkg.BfhipError as e:            # the VM refused the program: nothing was submitted
                    failed += 1
                    print(f"{path}: error: {e}", file=sys.stderr)
                    continue
                cols, ptrs = generic_columns(pkg, ctx, tr, a.log_max_rows)
                held[i] = (tr.log_sizes, ptrs)
                tr.close()
                try:
                    pool.submit_air(pkg.brainfuck_air_statement(held[i][0], a.log_max_rows, conv[2]), cols, ch, tag=i)
                except pkg.BfhipError as e:            # the validator refused the statement (a trace too large for --log-max-rows)
                    failed += 1
                    print(f"{path}: error: {e}", file=sys.stderr)
                    for p in held.pop(i)[1]:
                        ctx.free(p)
        for r in pool.as_completed(timeout_s=3600.0):
            path = a.programs[r.tag]
            log_sizes, ptrs = held.pop(r.tag)
            for p in ptrs:
                ctx.free(p)
            if not r.ok:
                failed += 1
                print(f"{path}: error: {r.error}", file=sys.stderr)
                continue
            proof = brainfuck_proof_of(r.proof, log_sizes)
            out = os.path.join(a.output_dir, os.path.splitext(os.path.basename(path))[0] + ".proof.json")
            open(out, "wb").write(proof)
            print(f"{out}  {len(proof)} bytes; queued {1e3 * r.seconds_queued:.1f} ms, proving {1e3 * r.seconds_proving:.1f} ms on worker {r.worker}; "
                  f"{time.time() - t0:.3f}s after the first submit", flush=True)
    finally:
        pool.close()
        for _, ptrs in held.values():
            for p in ptrs:
                ctx.free(p)
        ctx.close()
    return 1 if failed else 0


def generic_verify(pkg, proof, log_max_rows, conv, pcs):
    """(ok, reason) of a BrainfuckProof file through bfhip_air_verify under the statement that its claim describes"""
    import json
    try:
        full = json.loads(proof)
        log_sizes = [full["claim"][n]["log_size"] for n in pcs_replay.NAMES]
        sums = [full["interaction_claim"][n]["claimed_sum"] for n in pcs_replay.NAMES]
        member = pcs_replay.proof_member(proof)
    except (ValueError, KeyError, TypeError) as e:
        return False, "InvalidStructure: %s" % e
    if any(not isinstance(l, int) or l < 4 or l > log_max_rows for l in log_sizes):
        return False, "InvalidStructure: log_size"
    st = pkg.brainfuck_air_statement(log_sizes, log_max_rows, conv[2])
    with pkg.Channel(conv) as ch:
        return pkg.air_verify(st, b'{"claimed_sums":' + pcs_replay.compact(sums) + b',"proof":' + member + b"}", ch, conv, pcs)


def run(pkg, a, ap):
    if a.cmd == "prove" and a.generic and (a.all_sets or a.preflight):
        ap.error("--generic does not go with --all-sets or --preflight")
    if a.cmd == "prove" and a.queue:
        return prove_queue_generic(pkg, a, ap) if a.generic else prove_queue(pkg, a, ap)
    if a.cmd == "check":
        return check(pkg, a, ap)
    if a.cmd == "relations":
        return relations(pkg, a, ap)
    if a.cmd == "prove":
        code = open(a.file).read() if a.file else a.code
        if code is None:
            ap.error("prove needs --file or --code")
        inp = open(a.input_file, "rb").read() if a.input_file else (b"" if sys.stdin.isatty() else sys.stdin.buffer.read())
        sets = all_sets(channels=(0,)) if a.all_sets else [parse_conventions(a)]
        if a.all_sets:
            os.makedirs(a.all_sets, exist_ok=True)
        pcs = parse_pcs(pkg, a)
        ctx = pkg.Context(0, max_log_domain=a.log_max_rows + pcs.log_blowup_factor + 1)
        ctx.set_pcs_config(pcs)
        ctx.set_preflight(a.preflight)
        print(f"PcsConfig: pow_bits={pcs.pow_bits} log_blowup_factor={pcs.log_blowup_factor} n_queries={pcs.n_queries} "
              f"log_last_layer_degree_bound={pcs.log_last_layer_degree_bound}; security {pkg.security_bits(pcs)} bits", file=sys.stderr)
        t0 = time.time()
        if a.set_register or a.set_word:
            tr = pkg.Trace.from_registers(ctx, *executed_machine(pkg, a, ap, code, inp))
        else:
            tr = pkg.Trace(ctx, code, inp, ram_size=a.ram_size)
        t_prep = time.time() - t0           # VM run + table build + upload, once, whatever the number of convention sets
        for conv in sets:
            ctx.set_conventions(*conv)
            t_start = time.time()
            try:
                proof = generic_prove(pkg, ctx, tr, a.log_max_rows, conv)[0] if a.generic else tr.prove(a.log_max_rows)[0]
            except pkg.TraceRejected as e:          # --preflight: the lines check / relations would print
                print(e)
                tr.close(); ctx.close()
                return 1
            t_proof = time.time() - t_start
            print(f"Steps: {tr.n_steps}; trace preparation {1e3 * t_prep:.1f} ms; proof generation time: {t_proof:.3f}s; {len(proof)} bytes; {describe(conv)}", file=sys.stderr)
            if a.all_sets:
                path = os.path.join(a.all_sets, "proof_%d%d%d%d.json" % conv)
                open(path, "wb").write(proof)
                print(path)
            elif a.output:
                open(a.output, "wb").write(proof)
            else:
                sys.stdout.buffer.write(proof)
        tr.close(); ctx.close()
        return 0
    proof = open(a.proof, "rb").read()
    if a.try_all:
        accepted, reasons = try_all(pkg, proof, a.log_max_rows, parse_pcs(pkg, a))
        for conv in accepted:
            print("Proof verified under --conventions %d,%d,%d,%d  (%s)" % (conv + (describe(conv),)))
        if not accepted:
            print("Verification failed under every convention set; first failing check per set:")
            for conv, why in reasons.items():
                print("  %d,%d,%d,%d  %s" % (conv + (why,)))
        return 0 if accepted else 1
    conv = parse_conventions(a)
    if a.generic:
        ok, why = generic_verify(pkg, proof, a.log_max_rows, conv, parse_pcs(pkg, a))
    else:
        ok, why = pkg.verify_brainfuck(proof, a.log_max_rows, conventions=conv, pcs_config=parse_pcs(pkg, a))
    print("Proof verified" if ok else f"Verification failed: {why}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
