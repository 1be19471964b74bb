"""The Brainfuck protocol of mod.rs:471-735 / 738-797 replayed in Python over the commitment-scheme session of the product
(pkg.Channel, pkg.PcsSession, pkg.PcsVerifier): what tests/test_pcs_session_cpu.py (verifier side, oracle proofs) and
tests/test_gpu_pcs_session.py (prover side, captured polynomials) share. Nothing here knows a proof's bytes: the helpers only order
the calls — commit root0; mix the 13 log sizes; commit root1; three draw_felts(2); mix the 13 claimed sums; commit root2; draw_felts(1);
commit root3; draw_point — and describe the mask."""
import ctypes
import json

P = (1 << 31) - 1
# the keys of the claim, in claim order (mod.rs:85-99)
NAMES = ("memory", "instruction", "program", "processor", "jump_if_not_zero", "jump_if_zero", "input_instruction", "left_instruction", "minus_instruction",
         "output_instruction", "plus_instruction", "right_instruction", "end_of_execution")


def component_shapes(pkg):
    """[(n_main, n_logup)] of the 13 components (bfhip_component_shape)."""
    out = []
    for k in range(13):
        a, b, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        assert pkg.lib().bfhip_component_shape(k, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
        out.append((a.value, b.value))
    return out


def tree_log_sizes(pkg, log_sizes, log_max_rows):
    """Trace-domain log sizes of the columns of the four trees, in commit order."""
    shapes = component_shapes(pkg)
    t0 = list(range(log_max_rows, 3, -1))
    t1 = [log_sizes[k] for k in range(13) for _ in range(shapes[k][0])]
    t2 = [log_sizes[k] for k in range(13) for _ in range(4 * shapes[k][1])]
    t3 = [max(log_sizes) + 1] * 4
    return [t0, t1, t2, t3]


def mask_of(pkg, log_sizes, log_max_rows, oods, logup_mask_order):
    """(points, samples): point 0 = the out-of-domain point, point 1 + k = its shift by -1 trace step of component k
    (bfhip_circle_point_offset); samples[tree][column] = point indices — the `sp` of host/verifier.h."""
    shapes = component_shapes(pkg)
    points = [list(oods)] + [pkg.circle_point_offset(oods, log_sizes[k], -1) for k in range(13)]
    s0 = [[] for _ in range(log_max_rows - 3)]
    for k in range(13):
        s0[log_max_rows - log_sizes[k]] = [0]
    s1 = [[0] for k in range(13) for _ in range(shapes[k][0])]
    s2 = []
    for k in range(13):
        ni = 4 * shapes[k][1]
        for j in range(ni):
            if j + 4 >= ni:
                s2.append([1 + k, 0] if logup_mask_order == 1 else [0, 1 + k])
            else:
                s2.append([0])
    return points, [s0, s1, s2, [[0]] * 4]


def q_mul(x, y):
    """QM31 product: (a + b u)(c + d u) with u^2 = 2 + i over CM31 = M31[i]."""
    cm = lambda p, q: ((p[0] * q[0] - p[1] * q[1]) % P, (p[0] * q[1] + p[1] * q[0]) % P)
    ca = lambda p, q: ((p[0] + q[0]) % P, (p[1] + q[1]) % P)
    a, b, c, d = (x[0], x[1]), (x[2], x[3]), (y[0], y[1]), (y[2], y[3])
    bd = cm(b, d)
    lo = ca(cm(a, c), cm(bd, (2, 1)))
    hi = ca(cm(a, d), cm(b, c))
    return [lo[0], lo[1], hi[0], hi[1]]


def q_add(x, y):
    return [(x[k] + y[k]) % P for k in range(4)]


def from_partial_evals(v):
    """SecureField::from_partial_evals: v0 + v1 i + v2 u + v3 iu."""
    basis = ([1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1])
    r = [0, 0, 0, 0]
    for k in range(4):
        r = q_add(r, q_mul(v[k], basis[k]))
    return r


def flat_q(q):
    """serde form [[a, b], [c, d]] -> 4 words"""
    return [q[0][0], q[0][1], q[1][0], q[1][1]]


def root_bytes(h):
    """A commitment as the JSON carries it (32 byte values, or the felt252 as "0x.." hex) -> the 32 bytes the channel mixes."""
    if isinstance(h, str):
        return int(h, 16).to_bytes(32, "little")
    return bytes(h)


def compact(obj):
    return json.dumps(obj, separators=(",", ":")).encode()


def verify_replay(pkg, full, log_max_rows, conventions=(0, 0, 0, 0), pcs_config=None):
    """verify_brainfuck assembled from the session: full = the parsed BrainfuckProof. Returns (ok, reason) with the reasons of
    bfhip_verify_brainfuck_pcs. The structure checks in front of the channel replay are the caller's part of the protocol, as in stwo."""
    pf = full["proof"]
    if any(len(pf[k]) != 4 for k in ("commitments", "sampled_values", "decommitments", "queried_values")):
        return False, "InvalidStructure"
    log_sizes = [full["claim"][n]["log_size"] for n in NAMES]
    if any(l < 4 or l > log_max_rows for l in log_sizes):
        return False, "InvalidStructure: log_size"
    claimed = [flat_q(full["interaction_claim"][n]["claimed_sum"]) for n in NAMES]
    logs = tree_log_sizes(pkg, log_sizes, log_max_rows)
    ch, v = pkg.Channel(conventions), pkg.PcsVerifier(conventions, pcs_config)
    try:
        roots = [root_bytes(h) for h in pf["commitments"]]
        v.commit(ch, roots[0], logs[0])
        for l in log_sizes:
            ch.mix_u64(l)
        v.commit(ch, roots[1], logs[1])
        lookup = [w for _ in range(3) for q in ch.draw_felts(2) for w in q]
        if any(sum(c[k] for c in claimed) % P for k in range(4)):
            return False, "InvalidLookup: Invalid LogUp sum"
        for c in claimed:
            ch.mix_felts([c])
        v.commit(ch, roots[2], logs[2])
        random_coeff = ch.draw_felt()
        v.commit(ch, roots[3], logs[3])
        oods = ch.draw_point()
        points, samples = mask_of(pkg, log_sizes, log_max_rows, oods, conventions[2])
        sv = [[[flat_q(q) for q in col] for col in tree] for tree in pf["sampled_values"]]
        for t in range(4):
            if [len(c) for c in sv[t]] != [len(c) for c in samples[t]]:
                return False, "InvalidStructure: sampled_values"
        want = pkg.brainfuck_composition_at_point(log_sizes, claimed, log_max_rows, lookup, oods, sv, random_coeff, conventions)
        if from_partial_evals([sv[3][k][0] for k in range(4)]) != want:
            return False, "OodsNotMatching"
        return v.verify_values(ch, points, samples, compact(pf))
    finally:
        ch.close()
        v.close()


def proof_member(raw):
    """The bytes of the "proof" member of a BrainfuckProof's JSON (the last '}' closes the outer object)."""
    return raw[raw.index(b'"proof":') + len(b'"proof":'):-1]
