"""Child process of tests/test_gpu_fft.py::test_library_launches_what_the_plan_model_says. Started with BFHIP_FFT_PROF_DETAIL=1 in its
environment (the library reads the switch once per process): runs every transform of fft_plan_model.MANY_COLUMNS and LARGER_BLOWUPS alone,
with the per-launch profiler on, and prints one JSON line: [{"job": [inverse, log, src_log, ncols], "launches": {kernel name: calls}}].
The values transformed do not matter here (zeros); the parent compares the names with the model."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_plan_model as fm  # noqa: E402
from conftest import load_package  # noqa: E402


def main():
    assert os.environ.get("BFHIP_FFT_PROF_DETAIL") == "1"
    pkg = load_package()
    lib = pkg.lib()
    ctx = pkg.Context(0, max_log_domain=24)
    out = []

    def report():
        return {k: v["calls"] for k, v in ctx.profile_report().items() if k.startswith("k_fft")}

    def run(inverse, log, src_log, ncols):
        src = [ctx.malloc(4 << src_log) for _ in range(ncols)]
        dst = src if inverse else [ctx.malloc(4 << log) for _ in range(ncols)]
        for p in src:
            pkg._check(lib.bfhip_memset_zero(ctx._h, ctypes.c_void_p(p), ctypes.c_size_t(4 << src_log)))
        ctx.profile_reset()
        if inverse:
            ctx.interpolate(src, dst, log)
        else:
            ctx.evaluate(src, dst, src_log, log)
        ctx.sync()
        out.append({"job": [int(inverse), log, src_log, ncols], "launches": report()})
        for p in set(src + dst):
            ctx.free(p)

    try:
        ctx.profile_enable(1)
        for log, n in fm.MANY_COLUMNS:
            run(True, log, log, n)
        for log, n in fm.MANY_COLUMNS:
            run(False, log + 1, log, n)
        for log, log_eval, n in fm.LARGER_BLOWUPS:
            run(False, log_eval, log, n)
        ctx.profile_enable(0)
    finally:
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
