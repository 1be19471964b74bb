#!/usr/bin/env python3
"""What bringing a row-order trace into storage order costs: bfhip_columns_from_rows (and its inverse) beside (a) a device-to-device copy of
the same number of bytes on the same GPU — the ceiling for a kernel that reads and writes each word once — and (b) the route callers
had before: the test helper's numpy permutation per column plus the upload. In one run on one GPU.

  python3 tools/columns_rate.py [--passes 5] [--rounds 5] [--small] [--out FILE]

  cases      2^24 rows x 7 row-major (the register-row shape), 2^20 x 64 row-major, 2^22 x 16 column-major, and the inverse of the first
             (bfhip_rows_from_columns); full tables, identity column map, the table resident in HBM. --small: 2^16-row versions (a dry run).
  device     one call on resident device tables into resident columns, its read-back included: what a caller waits for. Also by HIP
             events (the library's profiler, scope k_columns_from_rows / k_rows_from_columns): the launch alone, and 8 bytes per word over it.
  copy       hipMemcpyAsync device to device of the table's bytes, then a wait for the device; GB/s counts the bytes read AND written, as
             for the kernel.
  numpy      per column: col[index] with the helper's index array precomputed (tests/test_gpu_air_program.py: _storage_of_coset_order),
             bfhip_upload into a fresh buffer, free. The inverse: bfhip_download per column, one fancy-indexed gather, a stack. Pageable
             numpy memory, one host thread. One call per window (it is long).
  time       ms per call: the three alternate in windows, `rounds` rounds (at least five) after a warm-up round (tools/ratelib.py).
  check      before the timing: the device's bytes equal the model's (tests/columns_model.py) and the numpy route's.

No threshold is attached. A run without a GPU fails: nothing here is measured on the host alone."""
import argparse
import ctypes
import statistics

import numpy as np

from ratelib import alternate, cell, emit, events, load_package, require_gpu

import columns_model as model      # tests/ (ratelib put it on the path)

P = (1 << 31) - 1
D2D = 3      # hipMemcpyDeviceToDevice


def measure(pkg, ctx, hip, a, log_size, n_cols, layout, inverse):
    n = 1 << log_size
    table = np.random.default_rng(log_size * 100 + n_cols).integers(0, P, size=(n, n_cols), dtype=np.uint32)
    index = model.rows_of_cells(log_size)
    want = model.columns_from_rows(table, log_size)
    ptrs = []
    try:
        cols = [ctx.malloc(4 * n) for _ in range(n_cols)]; ptrs += cols
        copy_dst = ctx.malloc(4 * n * n_cols); ptrs.append(copy_dst)
        if layout == "columns":
            src_cols = [ctx.upload(table[:, c]) for c in range(n_cols)]; ptrs += src_cols
            src, copy_src = pkg.DeviceRowColumns(src_cols, n), None
        else:
            rows = ctx.upload(table); ptrs.append(rows)
            src, copy_src = pkg.DeviceRows(rows, n, n_cols, n_cols), rows
        if copy_src is None:      # column-major: the copy reference moves the same bytes out of one buffer
            copy_src = ctx.upload(table); ptrs.append(copy_src)
        col_arr = (ctypes.c_void_p * n_cols)(*cols)

        def copy():
            assert hip.hipMemcpyAsync(ctypes.c_void_p(copy_dst), ctypes.c_void_p(copy_src), ctypes.c_size_t(4 * n * n_cols), D2D, None) == 0
            assert hip.hipDeviceSynchronize() == 0

        if not inverse:
            device = lambda: ctx.columns_from_rows(src, log_size, out=cols)

            def numpy_route():
                for c in range(n_cols):
                    ctx.free(ctx.upload(table[:, c][index]))

            device()
            got = np.stack([ctx.download(p, n) for p in cols])
            if got.tobytes() != want.tobytes() or np.stack([table[:, c][index] for c in range(n_cols)]).tobytes() != want.tobytes():
                raise SystemExit("columns_rate: the device, the model and the numpy route disagree at 2^%d x %d" % (log_size, n_cols))
            scope = "k_columns_from_rows"
        else:
            for p, c in zip(cols, want):
                pkg._check(pkg.lib().bfhip_upload(ctx._h, ctypes.c_void_p(p), c.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(c.nbytes)))
            cells = model.cells_of_rows(log_size)

            def device():
                pkg._check(pkg.lib().bfhip_rows_from_columns(ctx._h, col_arr, ctypes.c_uint32(n_cols), ctypes.c_uint32(log_size), ctypes.c_void_p(rows),
                                                              ctypes.c_uint64(n), ctypes.c_uint64(n_cols), ctypes.c_uint32(0)))
                ctx.sync()

            def numpy_route():
                numpy_route.last = np.stack([ctx.download(p, n)[cells] for p in cols], axis=1)

            pkg._check(pkg.lib().bfhip_memset_zero(ctx._h, ctypes.c_void_p(rows), ctypes.c_size_t(4 * n * n_cols)))
            device()
            numpy_route()
            if ctx.download(rows, n * n_cols).tobytes() != table.tobytes() or numpy_route.last.tobytes() != table.tobytes():
                raise SystemExit("columns_rate: the inverse, the model and the numpy route disagree at 2^%d x %d" % (log_size, n_cols))
            scope = "k_rows_from_columns"
        ms = alternate(ctx, {"device": device, "copy": copy}, a.passes, a.rounds)
        ms.update(alternate(ctx, {"numpy": numpy_route}, 1, a.rounds))
        ev = events(ctx, device, a.passes)[scope][0]
        return ms, ev
    finally:
        for p in ptrs:
            ctx.free(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=5); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--small", action="store_true"); ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("columns_rate: at least five rounds")
    pkg = load_package()
    require_gpu(pkg, "columns_rate")
    hip = ctypes.CDLL("libamdhip64.so")
    ctx = pkg.Context(0, max_log_domain=16)
    cases = [(24, 7, "rows", False), (20, 64, "rows", False), (22, 16, "columns", False), (24, 7, "rows", True)]
    if a.small:
        cases = [(16, c, l, inv) for _, c, l, inv in cases]
    lines = [f"bfhip_columns_from_rows / bfhip_rows_from_columns (device) beside a device-to-device copy of the table's bytes (copy) and beside the numpy "
             f"permutation per column plus upload, or download plus gather for the inverse (numpy): full tables resident in HBM, identity column map; {a.rounds} "
             f"alternating rounds of {a.passes} calls (numpy: 1 call) after a warm-up round, the context synchronised around every window; equal bytes "
             f"(device = model = numpy route) checked first. GB/s counts bytes read and written: 8 bytes per word.", "",
             "case | path | ms per call: median (min-max) | GB/s at the median | launch alone by HIP events: ms, GB/s"]
    try:
        for log_size, n_cols, layout, inverse in cases:
            ms, ev = measure(pkg, ctx, hip, a, log_size, n_cols, layout, inverse)
            traffic = 8.0 * n_cols * (1 << log_size)
            med = {k: statistics.median(v) for k, v in ms.items()}
            name = "2^%d x %d %s%s" % (log_size, n_cols, "row-major" if layout == "rows" else "column-major", ", inverse" if inverse else "")
            for path in ("device", "copy", "numpy"):
                by_events = "%.4f, %.0f" % (ev, traffic / ev / 1e6) if path == "device" else "-"
                lines.append(f"{name} | {path} | {cell(ms[path], 4)} | {traffic / med[path] / 1e6:.1f} | {by_events}")
            lines += [f"{name} | device / copy (median ms) | {med['device'] / med['copy']:.2f}x; launch alone / copy {ev / med['copy']:.2f}x",
                      f"{name} | numpy / device (median ms) | {med['numpy'] / med['device']:.1f}x", ""]
    finally:
        ctx.close()
    emit("\n".join(lines), a.out)


if __name__ == "__main__":
    main()
