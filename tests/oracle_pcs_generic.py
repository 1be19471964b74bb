"""ctypes view of tests/native/oracle_pcs_generic.cpp: the CPU oracle's commitment scheme over arbitrary columns — a channel, and a session
that commits trees (interpolate_col + commit_tree) and opens them (orc::Prover::prove_values) under the description PcsSession.prove_values
takes. Built with g++ into a temporary directory by the `gshim` fixtures of tests/test_pcs_generic_oracle_cpu.py and
tests/test_gpu_pcs_generic_oracle.py. Channel and Session mirror pkg.Channel and pkg.PcsSession method for method, so that one replay
(tests/pcs_replay.py, tests/pcs_generic_cases.py) drives either side."""
import ctypes
import os
import subprocess
import time

import numpy as np

import pcs_generic_cases as gc
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "oracle_pcs_generic.cpp")


def build(directory):
    path = os.path.join(str(directory), "liboracle_pcs_generic.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-I", os.path.join(ROOT, "oracle"), "-o", path, SRC,
                           os.path.join(ROOT, "oracle", "simd_port.cpp"), "-lpthread"])
    return OraclePcsGeneric(path)


def _u32s(values):
    return (ctypes.c_uint32 * max(1, len(values)))(*[int(v) for v in values])


class OraclePcsGeneric:
    def __init__(self, path):
        self.L = L = ctypes.CDLL(path)
        L.opg_last_error.restype = ctypes.c_char_p
        L.opg_channel_new.restype = ctypes.c_void_p
        L.opg_session_new.restype = ctypes.c_void_p
        L.opg_channel_state.restype = None
        for name in ("opg_channel_free", "opg_session_free", "opg_free"):
            getattr(L, name).restype = None
            getattr(L, name).argtypes = [ctypes.c_void_p]
        # OpenMP over every hardware thread of a large host is slower than a few threads for these sizes
        L.opg_set_threads(min(os.cpu_count() or 1, 16))

    def _chk(self, rc):
        if rc < 0:
            raise RuntimeError(self.L.opg_last_error().decode())
        return rc

    def set_conventions(self, merkle_node_hash=0, mix_u64=0, logup_mask_order=0, merkle_channel=0):
        """Process-wide in the shim. A Channel takes its kind from them when it is created."""
        self._chk(self.L.opg_set_conventions(merkle_node_hash, mix_u64, logup_mask_order, merkle_channel))

    def Channel(self):
        return Channel(self)

    def Session(self, pow_bits=5, log_blowup_factor=1, n_queries=3, max_log_size=20):
        return Session(self, pow_bits, log_blowup_factor, n_queries, max_log_size)


class Channel:
    """orc::Channel under the shim's conventions at this moment; the methods of pkg.Channel."""

    def __init__(self, shim):
        self.shim, self._h = shim, ctypes.c_void_p(shim.L.opg_channel_new())

    def close(self):
        if self._h:
            self.shim.L.opg_channel_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def mix_root(self, hash32):
        hash32 = bytes(hash32)
        assert len(hash32) == 32
        self.shim._chk(self.shim.L.opg_channel_mix_root(self._h, hash32))

    def mix_u64(self, value):
        self.shim._chk(self.shim.L.opg_channel_mix_u64(self._h, ctypes.c_uint64(int(value))))

    def mix_felts(self, felts):
        flat = [int(w) for q in felts for w in q]
        assert len(flat) == 4 * len(felts)
        self.shim._chk(self.shim.L.opg_channel_mix_felts(self._h, _u32s(flat), ctypes.c_size_t(len(felts))))

    def draw_felts(self, n=1):
        out = (ctypes.c_uint32 * (4 * max(1, n)))()
        self.shim._chk(self.shim.L.opg_channel_draw_felts(self._h, ctypes.c_size_t(n), out))
        return [[int(out[4 * i + k]) for k in range(4)] for i in range(n)]

    def draw_felt(self):
        return self.draw_felts(1)[0]

    def draw_point(self):
        out = (ctypes.c_uint32 * 8)()
        self.shim._chk(self.shim.L.opg_channel_draw_point(self._h, out))
        return [int(v) for v in out]

    def state(self):
        """(digest bytes, n_sent)"""
        d, n = (ctypes.c_uint8 * 32)(), ctypes.c_uint32()
        self.shim.L.opg_channel_state(self._h, d, ctypes.byref(n))
        return bytes(d), n.value


class Session:
    """Trees of host columns (numpy uint32 arrays) under an explicit PcsConfig; commit and prove_values as pkg.PcsSession has them."""

    def __init__(self, shim, pow_bits, log_blowup_factor, n_queries, max_log_size):
        self.shim = shim
        self._h = ctypes.c_void_p(shim.L.opg_session_new(pow_bits, log_blowup_factor, n_queries, max_log_size))
        if not self._h:
            raise RuntimeError(shim.L.opg_last_error().decode())
        self.n_cols = []

    def close(self):
        if self._h:
            self.shim.L.opg_session_free(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def commit(self, channel, cols, log_sizes, form=0):
        """The root (32 bytes), mixed into `channel`."""
        assert len(cols) == len(log_sizes)
        keep = [np.ascontiguousarray(c, dtype=np.uint32) for c in cols]
        assert all(c.shape == (1 << l,) for c, l in zip(keep, log_sizes))
        ptrs = (ctypes.c_void_p * max(1, len(keep)))(*[c.ctypes.data for c in keep])
        root = (ctypes.c_uint8 * 32)()
        self.shim._chk(self.shim.L.opg_session_commit(self._h, channel._h, ptrs, _u32s(log_sizes), len(keep), int(form), root))
        self.n_cols.append(len(keep))
        return bytes(root)

    def prove_values(self, channel, points, samples, with_sampled=False):
        """samples[tree][column] = indices into points, in sample order. Returns the CommitmentSchemeProof's serde bytes (and, with_sampled,
        the sampled values flat as 4-word lists)."""
        assert [len(t) for t in samples] == self.n_cols
        counts = [len(col) for tree in samples for col in tree]
        idx = [int(i) for tree in samples for col in tree for i in col]
        flat = [int(w) for p in points for w in p]
        assert len(flat) == 8 * len(points)
        out = (ctypes.c_uint32 * (4 * max(1, len(idx))))()
        js, n = ctypes.c_void_p(), ctypes.c_size_t()
        self.shim._chk(self.shim.L.opg_session_prove_values(self._h, channel._h, _u32s(flat), len(points), _u32s(counts), _u32s(idx), out,
                                                            ctypes.byref(js), ctypes.byref(n)))
        proof = ctypes.string_at(js, n.value)
        self.shim.L.opg_free(js)
        if with_sampled:
            return proof, [[int(out[4 * i + k]) for k in range(4)] for i in range(len(idx))]
        return proof


def prove_case(shim, pkg, case, columns=None, form=None):
    """A case of tests/pcs_generic_cases.py on the shim: (roots, drawn point, points, proof, sampled values, channel state, seconds).
    columns / form: other columns than the case's own, committed in another form (the `forms` case)."""
    shim.set_conventions(*case.conv)
    try:
        ch = shim.Channel()
        t0 = time.perf_counter()
        with shim.Session(max_log_size=case.max_log, **case.cfg) as s:
            out = gc.prove(case, pkg, s, ch, case.columns() if columns is None else columns, form=form)
        return out + (ch.state(), time.perf_counter() - t0)
    finally:
        shim.set_conventions(0, 0, 0, 0)
