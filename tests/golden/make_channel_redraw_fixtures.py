"""Writes channel_redraw.json: channel states at which Blake2sChannel::draw_felt REJECTS its first draw (one of the 8 words is >= 2P, i.e.
0xFFFFFFFE or 0xFFFFFFFF: 2^-28 per draw) at a chosen step of the FRI commit phase. A proof takes that branch about once in 10^7, so the
tests that pin it (tests/test_oracle_math.py, tests/test_gpu_fri_commit.py) need inputs found by search.

    python tests/golden/make_channel_redraw_fixtures.py [R0 R1 ..]      (needs oracle/libbforacle.so; 8 processes, a few minutes)

The search walks a counter, against tests/fri_commit_model.py (hashlib): a try at step j is j + 1 mix_root hashes and one draw.
  R0  a root: on the zero digest, mix_root(root) then draw_felt rejects its first draw                       (the oracle's own retry)
  R1  an initial digest: line_log 12, uniform columns of every size; rejection at step 0 (the first-layer tree's root needs no alpha)
  R2  line_log 12, rejection at step 2 (the 2^11-row layer)
  R3, R4  line_log 10, rejection at step 1 and at step 2
R2 to R4 fold ONE constant column ("largest only"): every layer is then constant whatever the alphas are, so every root is known before the
search and a try is pure hashing. That independence is asserted below, not assumed.
Every found state is run through the whole model: exactly the chosen step redraws, once, and no other step does."""
import ctypes
import json
import multiprocessing
import os
import struct
import sys
import time
from hashlib import blake2s

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np

import fri_commit_model as model

P = (1 << 31) - 1
OUT = os.path.join(HERE, "channel_redraw.json")
LOG_BLOWUP = 1
CONSTANT = (1234567, 7654321, P - 1, 5)          # the constant column of R2 .. R4 (one QM31 value)
CHUNK = 1 << 20
Z32 = bytes(32)
TAG = b"bfhip channel redraw\0\0\0\0"            # 24 bytes: candidate = TAG || LE64(counter)
FIXTURES = {"R0": (None, 0), "R1": (12, 0), "R2": (12, 2), "R3": (10, 1), "R4": (10, 2)}      # name: (line_log, rejecting step)


def uniform_every_size(line_log):
    """The data of the GPU test's ("uniform", "every size") case: tests/test_gpu_fri_commit.py builds it through the same two calls."""
    import field_inputs as fi
    return model.quotient_columns(fi.FAMILIES["uniform"], model.pattern_sizes("every", line_log, LOG_BLOWUP))


def constant_largest_only(line_log):
    n = 2 << line_log
    return [(line_log + 1, [np.full(n, c, dtype=np.uint32) for c in CONSTANT])]


def _scan(job):
    """First counter in [lo, hi) whose candidate makes the draw behind the last of `roots` reject, or None. fixed_digest: the candidate is the
    (single) root mixed into that digest (R0); otherwise the candidate is the initial digest."""
    lo, hi, roots, fixed_digest = job
    for counter in range(lo, hi):
        cand = TAG + struct.pack("<Q", counter)
        if fixed_digest is not None:
            d = blake2s(fixed_digest + cand).digest()
        else:
            d = cand
            for r in roots:
                d = blake2s(d + r).digest()
        w = blake2s(d + Z32).digest()
        if b"\xff\xff\xff" in w and any(x >= 2 * P for x in struct.unpack("<8I", w)):
            return counter
    return None


def search(pool, roots, fixed_digest, start=0):
    lo = start
    while True:
        jobs = [(lo + k * CHUNK, lo + (k + 1) * CHUNK, roots, fixed_digest) for k in range(64)]
        for hit in pool.imap(_scan, jobs):      # in order: the smallest counter wins, whatever the number of processes
            if hit is not None:
                return hit
        lo += 64 * CHUNK


def make(name, pool, L):
    line_log, step = FIXTURES[name]
    t0 = time.time()
    if name == "R0":
        counter = search(pool, None, Z32)
        root = TAG + struct.pack("<Q", counter)
        digest = model.mix_root(Z32, root)
        first = model.draw_words(digest, 0)
        alpha, n_sent = model.draw_felt(digest)
        assert any(x >= 2 * P for x in first) and n_sent == 2
        return {"root": root.hex(), "first_draw": [int(x) for x in first], "n_sent": n_sent, "alpha": alpha, "tries": counter + 1, "search_seconds": round(time.time() - t0, 1)}
    data = uniform_every_size(line_log) if name == "R1" else constant_largest_only(line_log)
    ref = model.commit(L, data, LOG_BLOWUP, Z32)
    if name != "R1":
        other = model.commit(L, data, LOG_BLOWUP, bytes(range(32)))
        assert other["roots"] == ref["roots"] and not np.array_equal(other["alphas"], ref["alphas"]), "the roots of a constant column must not depend on the alphas"
        assert all(np.array_equal(a, b) for a, b in zip(other["layers"], ref["layers"]))
    roots = ref["roots"][:step + 1]      # R1: roots[0] is the first-layer tree's, computed before any alpha exists
    start = 0
    while True:
        counter = search(pool, roots, None, start)
        digest = TAG + struct.pack("<Q", counter)
        got = model.commit(L, data, LOG_BLOWUP, digest)
        if got["draws"] == [2 if k == step else 1 for k in range(len(got["draws"]))]:
            break
        start = counter + 1              # another step redraws too, or the redraw is rejected again: not the fixture wanted
    assert got["roots"][:step + 1] == roots
    return {"line_log": line_log, "step": step, "digest": digest.hex(), "n_sent": 2, "alpha": [int(x) for x in got["alphas"][step]],
            "final_digest": got["digest"].hex(), "final_n_sent": got["n_sent"], "tries": counter + 1, "search_seconds": round(time.time() - t0, 1)}


def main():
    names = sys.argv[1:] or list(FIXTURES)
    L = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "libbforacle.so"))
    L.orc_last_error.restype = ctypes.c_char_p
    out = json.load(open(OUT)) if os.path.exists(OUT) else {}
    out["_note"] = "made by make_channel_redraw_fixtures.py; search_seconds: wall time of the search with 8 processes"
    with multiprocessing.Pool(8) as pool:
        for name in names:
            out[name] = make(name, pool, L)
            print(name, out[name], flush=True)
            json.dump(out, open(OUT, "w"), indent=1, sort_keys=True)
            open(OUT, "a").write("\n")


if __name__ == "__main__":
    main()
