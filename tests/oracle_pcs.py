"""ctypes view of tests/native/oracle_pcs.cpp: the CPU oracle (the checker) proving and verifying under an explicit PcsConfig.
Built with g++ into a temporary directory by the `oracle_pcs` fixtures of tests/test_pcs_config_cpu.py and tests/test_gpu_pcs_config.py.
Its proofs are the byte-exact reference at every log_blowup_factor (above 1 the oracle evaluates the constraints on their own domain, see the
source's header)."""
import ctypes
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "oracle_pcs.cpp")


def build(directory):
    path = os.path.join(str(directory), "liboracle_pcs.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-I", os.path.join(ROOT, "oracle"), "-o", path, SRC,
                           os.path.join(ROOT, "oracle", "simd_port.cpp"), "-lpthread"])
    return OraclePcs(path)


class OraclePcs:
    def __init__(self, path):
        self.L = ctypes.CDLL(path)
        self.L.ops_last_error.restype = ctypes.c_char_p

    def _chk(self, rc):
        if rc < 0:
            raise RuntimeError(self.L.ops_last_error().decode())
        return rc

    def set_conventions(self, merkle_node_hash=0, mix_u64=0, logup_mask_order=0, merkle_channel=0):
        self._chk(self.L.ops_set_conventions(merkle_node_hash, mix_u64, logup_mask_order, merkle_channel))

    def prove(self, code, inp=b"", log_max_rows=20, pow_bits=5, log_blowup_factor=1, n_queries=3):
        """(proof JSON bytes, {tap name: hex digest})"""
        js, n, tr = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_void_p()
        self._chk(self.L.ops_prove(code.encode(), inp, ctypes.c_size_t(len(inp)), log_max_rows, pow_bits, log_blowup_factor, n_queries,
                                   ctypes.byref(js), ctypes.byref(n), ctypes.byref(tr)))
        proof = ctypes.string_at(js, n.value)
        taps = ctypes.string_at(tr).decode()
        self.L.ops_free(js)
        self.L.ops_free(tr)
        return proof, dict(line.split(":") for line in taps.strip().split("\n"))

    def taps(self, code, inp=b"", log_max_rows=20, pow_bits=5, log_blowup_factor=1, n_queries=3):
        """The transcript taps of the oracle's proof under this config."""
        return self.prove(code, inp, log_max_rows, pow_bits, log_blowup_factor, n_queries)[1]

    def verify(self, js, log_max_rows=20, pow_bits=5, log_blowup_factor=1, n_queries=3):
        err = ctypes.create_string_buffer(512)
        rc = self._chk(self.L.ops_verify(js, ctypes.c_size_t(len(js)), log_max_rows, pow_bits, log_blowup_factor, n_queries, err, ctypes.c_size_t(512)))
        return rc == 0, err.value.decode()
