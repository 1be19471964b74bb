"""The case matrix of the commitment-scheme session over arbitrary columns, shared by tests/test_pcs_generic_oracle_cpu.py (the oracle's
proof of every case is accepted by the library's host verifier) and tests/test_gpu_pcs_generic_oracle.py (the session's proof of every case
is the oracle's, byte for byte). A case gives: trees of columns (trace-domain log size, family of tests/field_inputs.py, seed), the commit
form, the PcsConfig, the conventions, the sample points (the point drawn after the last commit, shifted by `offset` steps of the trace
domain of 2^log rows) and, per column, the point indices in sample order. Everything is deterministic; nothing here knows a proof's bytes.

The protocol of a case is the smallest one: commit every tree in order, draw the point, prove_values. `prove` drives it over any pair of
(session, channel) with the methods of pkg.PcsSession / pkg.Channel — the library's on device pointers, the oracle shim's
(tests/oracle_pcs_generic.py) on numpy columns.

Sizes are the smallest that reach each launch path (LDE level = log size + log_blowup_factor): the Merkle plan changes at levels 9 / 10 / 11 /
17 / 18, the FRI commit phase at line layers of 2^10 (tail), 2^11..2^16 (layer kernel) and 2^17 (fold inside the leaf launch)."""
import json
import random

import numpy as np

import field_inputs as fi
from conftest import P

STWO, RFC7693, MIX_U64, FLIPPED, POSEIDON = (0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 1, 0), (0, 0, 0, 1)
OODS = (1, 0)            # a point description (log, offset): the drawn point itself
MAX_LOG_DOMAIN = 20      # the largest LDE of the matrix: 19 + 1 (`wide20`); the `deep` cases end at 17 + 1 and 16 + 2


def column(log, family, seed):
    """One column of 2^log canonical words. Beside the families of field_inputs: `zero`, `const` (one value everywhere) and `lowhalf`
    (uniform, upper half zero: a coefficient column of half the degree)."""
    n = 1 << log
    if family == "zero":
        return np.zeros(n, dtype=np.uint32)
    if family == "const":
        return np.full(n, int(fi.column("uniform", seed, 1)[0]), dtype=np.uint32)
    if family == "lowhalf":
        v = fi.column("uniform", seed, n).copy()
        v[n // 2:] = 0
        return v
    return fi.column(family, seed, n)


class Case:
    def __init__(self, name, trees, samples, points=(OODS,), cfg=None, conv=STWO, form=0, seed=0, reaches=""):
        """trees[t] = [log or (log, family) or (log, family, seed)]; a bare log is a uniform column; a seed is given only to repeat a column."""
        self.name, self.conv, self.form, self.reaches = name, tuple(conv), form, reaches
        self.cfg = dict(dict(pow_bits=4, log_blowup_factor=1, n_queries=6), **(cfg or {}))
        self.points, self.samples = [tuple(p) for p in points], [[list(c) for c in t] for t in samples]
        base = 0x9C5 * 1000 + 7919 * (seed or sum(ord(ch) for ch in name))
        self.trees, k = [], 0
        for t in trees:
            cols = []
            for c in t:
                c = (c, "uniform") if isinstance(c, int) else tuple(c)
                k += 1
                cols.append((c[0], c[1], c[2] if len(c) > 2 else base + k))
            self.trees.append(cols)
        self.logs = [[c[0] for c in t] for t in self.trees]
        self.check()

    def check(self):
        """A description the session accepts: at most 2 samples per column, at most 64 points, sizes within [4, max_log_domain - blowup]."""
        b = self.cfg["log_blowup_factor"]
        assert [len(t) for t in self.samples] == [len(t) for t in self.trees], self.name
        assert all(len(c) <= 2 and all(0 <= i < len(self.points) for i in c) for t in self.samples for c in t), self.name
        assert 1 <= len(self.points) <= 64 and all(4 <= l <= MAX_LOG_DOMAIN - b for t in self.logs for l in t), self.name
        assert self.cfg["pow_bits"] <= (12 if self.conv[3] == 1 else 32) and 1 <= self.cfg["n_queries"] <= 256, self.name

    @property
    def max_log(self):
        return max(l for t in self.logs for l in t)

    def columns(self):
        """[tree][column] = np.uint32 array; equal descriptions give the same array object (a device column passed twice)."""
        made = {}
        return [[made.setdefault(c, column(*c)) for c in t] for t in self.trees]

    def points_at(self, pkg, oods):
        return [list(oods) if (log, off) == OODS else pkg.circle_point_offset(oods, log, off) for log, off in self.points]

    def __repr__(self):
        return self.name


def prove(case, pkg, session, ch, columns, form=None):
    """(roots, drawn point, points, proof bytes, sampled values flat) — columns[t][c] = what session.commit takes for a column; form: None =
    the case's own."""
    form = case.form if form is None else form
    roots = [session.commit(ch, columns[t], case.logs[t], form=form) for t in range(len(case.trees))]
    oods = ch.draw_point()
    points = case.points_at(pkg, oods)
    proof, sampled = session.prove_values(ch, points, case.samples, with_sampled=True)
    return roots, oods, points, proof, sampled


def verify(case, pkg, roots, proof, samples=None):
    """((ok, reason), drawn point, channel state) of pkg.PcsVerifier over the case's protocol."""
    ch, v = pkg.Channel(case.conv), pkg.PcsVerifier(case.conv, pkg.PcsConfig(**case.cfg))
    try:
        for t, root in enumerate(roots):
            v.commit(ch, root, case.logs[t])
        oods = ch.draw_point()
        return v.verify_values(ch, case.points_at(pkg, oods), case.samples if samples is None else samples, proof), oods, ch.state()
    finally:
        v.close()
        ch.close()


def members(proof_json):
    """The members of a CommitmentSchemeProof in the order the prover produces them: [(name, value)]."""
    pf = json.loads(proof_json)
    fri = pf["fri_proof"]
    out = [("commitments[%d]" % t, h) for t, h in enumerate(pf["commitments"])]
    for t, tree in enumerate(pf["sampled_values"]):
        out.append(("sampled_values[%d] (columns)" % t, len(tree)))
        for c, col in enumerate(tree):
            out.append(("sampled_values[%d][%d] (samples)" % (t, c), len(col)))
            out += [("sampled_values[%d][%d][%d]" % (t, c, k), q) for k, q in enumerate(col)]
    out.append(("fri_proof.first_layer.commitment", fri["first_layer"]["commitment"]))
    out.append(("fri_proof.inner_layers (count)", len(fri["inner_layers"])))
    out += [("fri_proof.inner_layers[%d].commitment" % i, l["commitment"]) for i, l in enumerate(fri["inner_layers"])]
    out.append(("fri_proof.last_layer_poly", fri["last_layer_poly"]))
    out.append(("proof_of_work", pf["proof_of_work"]))
    out += [("queried_values[%d]" % t, v) for t, v in enumerate(pf["queried_values"])]
    out += [("decommitments[%d]" % t, d) for t, d in enumerate(pf["decommitments"])]
    for name, l in [("first_layer", fri["first_layer"])] + [("inner_layers[%d]" % i, l) for i, l in enumerate(fri["inner_layers"])]:
        out.append(("fri_proof.%s.fri_witness" % name, l["fri_witness"]))
        out.append(("fri_proof.%s.decommitment" % name, l["decommitment"]))
    return out


def first_difference(got, want):
    """None when the two proofs are the same bytes; otherwise the name of the first member, in prover order, that differs."""
    if got == want:
        return None
    try:
        a, b = members(got), members(want)
    except Exception as e:          # not a proof at all
        return "unparsable: %r" % (e,)
    for (na, va), (nb, vb) in zip(a, b):
        if na != nb:
            return "structure: %s against %s" % (na, nb)
        if va != vb:
            return "%s: %r against %r" % (na, _short(va), _short(vb))
    return "length or serialisation: %d against %d bytes, every member equal" % (len(got), len(want))


def _short(v):
    s = json.dumps(v, separators=(",", ":"))
    return s if len(s) <= 160 else s[:157] + "..."


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------------
def _all(trees, idx=(0,)):
    return [[list(idx) for _ in t] for t in trees]


def _points64():
    """The drawn point and 63 shifts of it: odd offsets at seven sizes are 63 different multiples of the generator (odd / 2^log is in lowest
    terms, and -1, -3, -5 stay apart from 1 .. 11 from 2^5 up). Index order shuffled: not the order of the map that batches them."""
    pts = [OODS] + [(log, off) for log in (5, 6, 7, 8, 9, 10, 11) for off in (1, -1, 3, -3, 5, 7, -5, 9, 11)]
    random.Random(64).shuffle(pts)
    logs = [8] * 12 + [6] * 16 + [5] * 12
    # columns 0 .. 23 are opened at two points, 24 .. 39 at one: 64 samples, every point once; the scramble spreads the points over the sizes
    order = list(range(64))
    random.Random(65).shuffle(order)
    samples = [[order[2 * c], order[2 * c + 1]] for c in range(24)] + [[order[48 + c]] for c in range(16)]
    mix = list(range(40))
    random.Random(66).shuffle(mix)          # which column gets which sample list
    trees = [logs[:15], logs[15:]]
    flat = [samples[mix[c]] for c in range(40)]
    return trees, [flat[:15], flat[15:]], pts


def _wide20():
    """One tree above LDE level 18: 17 columns of 2^19 rows (tests/fft_plan_model.py: the count at which a workgroup of the LDE walks 2 columns
    and the last one 1) among the smaller sizes of tests/test_gpu_pcs_commit_large.py, in shuffled caller order. Every third column is opened
    at both points, the others at one of the two."""
    cols = [19] * 17 + [5, 9, 13, (16, "edge"), (13, "max"), (9, "zero"), (16, "const")]
    cols[1], cols[16] = (19, "max"), (19, "edge")
    random.Random(20).shuffle(cols)
    return [cols], [[[0, 1] if k % 3 == 0 else [1] if k % 3 == 1 else [0] for k in range(len(cols))]]


def _mid(name, cfg=None, conv=STWO, reaches=""):
    """The mid-size case of the `conventions` and `configs` rows: largest log 11, three sizes, two points. One seed: the same columns."""
    trees = [[11, 9, 9], [7, 11, 9]]
    return Case(name, trees, [[[0], [0, 1], [1, 0]], [[0], [0], [1]]], points=[OODS, (9, -1)], cfg=cfg, conv=conv, seed=1109, reaches=reaches)


def _cases():
    c = []
    t = [[4, 4, 4]]
    c.append(Case("tiny", t, _all(t), cfg=dict(n_queries=40, pow_bits=0),
                  reaches="top kernel from the leaves, tail-only FRI, more queries than the 32 rows, zero-bit grind"))
    t = [[5, 4]]
    c.append(Case("tail8", t, _all(t), cfg=dict(log_blowup_factor=3), reaches="FRI tail ending at 8 rows"))
    t = [[9, 9, 7, 4]]
    c.append(Case("level10", t, _all(t), reaches="deepest LDE level exactly 10"))
    t = [[10, 8], [10, 5]]
    c.append(Case("sub11", t, _all(t), reaches="lowest subtree launch"))
    t = [[16, 12], [7, 16]]
    c.append(Case("sub17", t, _all(t), reaches="highest subtree launch"))
    t = [[9, 16, 4, 12], [15, 5, 10, 7, 13], [6, 14, 8, 11]]
    s = _all(t)
    s[0][3], s[1][2], s[2][1] = [0, 1], [1, 0], [1]
    c.append(Case("ladder", t, s, points=[OODS, (12, -1)], reaches="13 size groups: a quotient folded into every FRI layer; layer kernel and tail"))
    t = [[17, 12, 9, 5]]
    c.append(Case("deep_b1", t, _all(t), reaches="single-level launches above the subtree; first FRI layer through the leaf launch"))
    t = [[16, 6]]
    c.append(Case("deep_b2", t, _all(t), cfg=dict(log_blowup_factor=2), reaches="the same at log_blowup_factor 2"))
    t, s = _wide20()
    c.append(Case("wide20", t, s, points=[OODS, (19, -1)],
                  reaches="17 columns of 2^19 rows: 2 columns per workgroup with a shorter last block in the LDE to level 20 (wide strided pass), "
                          "sampling and quotients over a many-column class of 2^20 rows, the FRI commit from 2^19; oracle: commit 0.36 s, prove_values 0.60 s on 8 threads"))
    for n in range(1, 14):
        t = [[6] * n + [8]]
        c.append(Case("batch%02d" % n, t, _all(t), reaches="%d columns in one batch: residue %d of the three-at-a-time loop" % (n, n % 3)))
    t = [[5] * 300 + [7, 7]]
    c.append(Case("wide", t, _all(t), reaches="more than 256 columns in a tree and in a size group"))
    t, s, pts = _points64()
    c.append(Case("points64", t, s, points=pts, reaches="the 64-point cap; batch order against index order"))
    t = [[6, 6, 6, 6, 5], [7, 6]]
    c.append(Case("equal_points", t, [[[0, 1], [2], [1, 0], [0], [0]], [[3, 0], [2]]], points=[OODS, (6, -1), (6, -1), (7, 3)],
                  reaches="two indices holding one point; [i, j] beside [j, i]"))
    t = [[8, 6, 6, 5], [6, 8]]
    c.append(Case("empty_middle", t, [[[0], [], [], [0]], [[], [0, 1]]], points=[OODS, (8, -1)], reaches="n_batches == 0 in the grouped launch"))
    c.append(Case("empty_largest", t, [[[], [0], [0, 1], [0]], [[1], []]], points=[OODS, (6, -1)], reaches="n_batches == 0 in the early launch"))
    t = [[(7, "uniform", 4401), 7, 6, (5, "lowhalf"), (7, "uniform", 4401)], [(6, "lowhalf"), 5]]
    c.append(Case("forms", t, [[[0], [0, 1], [0], [0], [1, 0]], [[0], [0]]], points=[OODS, (7, -1)], form=1,
                  reaches="coefficients and evaluations of the same polynomials; a half-degree column; one column twice"))
    t = [[(6, "max"), (6, "zero"), (6, "const"), (6, "edge"), 6, 6], [(8, "max"), 8, (5, "zero"), (8, "edge"), (5, "const")]]
    c.append(Case("values", t, [[[0], [0], [0, 1], [1, 0], [0], [1]], [[0], [0], [0], [0, 1], [0]]], points=[OODS, (6, -1)],
                  reaches="p - 1, zero, constant and edge columns beside uniform ones"))
    c.append(_mid("conv_stwo"))
    c.append(_mid("conv_rfc7693", conv=RFC7693, reaches="RFC 7693 node hashes"))
    c.append(_mid("conv_mix_u64", conv=MIX_U64, cfg=dict(pow_bits=9), reaches="the other mix_u64: the nonce is mixed with it"))
    c.append(_mid("conv_flipped", conv=FLIPPED, reaches="every switch on its other value"))
    c.append(_mid("conv_poseidon252", conv=POSEIDON, cfg=dict(pow_bits=7), reaches="Poseidon252 channel and tree"))
    for b in (1, 2, 3, 4):
        c.append(_mid("cfg_blowup%d" % b, cfg=dict(log_blowup_factor=b)))
    for q in (1, 3, 64):
        c.append(_mid("cfg_queries%d" % q, cfg=dict(n_queries=q)))
    for w in (0, 10, 16):
        c.append(_mid("cfg_pow%d" % w, cfg=dict(pow_bits=w)))
    assert len({k.name for k in c}) == len(c)
    return c


CASES = _cases()
BY_NAME = {k.name: k for k in CASES}
# the small cases the mutant and sanitizer tests use
SMALL = ("equal_points", "tail8")
assert P == (1 << 31) - 1
