#!/usr/bin/env python3
"""What deriving a table from a row-order trace by a filter and / or a sort costs on the device: bfhip_rows_select beside (a) a
device-to-device copy of the OUTPUT's bytes, (b) bfhip_columns_from_rows of as many rows unpermuted into the same columns — the gather
without the scatter of its reads —, and (c) the route an author had before: download the table, numpy boolean indexing / numpy.lexsort,
the storage-order permutation per column, upload. In one run on one GPU.

  python3 tools/rows_select_rate.py [--passes 5] [--rounds 5] [--small] [--out FILE]

  shapes     2^20 and 2^24 rows x 7 words, row-major and column-major, resident in HBM. Column 0 holds each of 0..7 exactly n / 8 times in
             random order, column 1 random values below 1024, the others random canonical words. --small: 2^14 and 2^16 rows (a dry run).
  selections filter: column 0 == 3 (one row in eight, S = n / 8 exactly) in source order; sort: every row ordered by (column 1, column 2);
             filter + sort: both. All 7 columns are written, offset 0, into the smallest domain that holds S.
  select     one bfhip_rows_select call into resident columns, both read-backs included: what a caller waits for, on a context with a
             scratch reserve (bfhip_ctx_set_scratch_reserve, --reserve-mib), so that the call allocates nothing. `select, no reserve` is
             the same call on a second context without one: seven device allocations and releases per call. By HIP events (the
             library's profiler) the call with the reserve splits into k_select_flags (flags, scan), rows_select_sort (key gathers and radix sorts)
             and k_select_gather; GB/s of the gather = its algorithmic bytes (8 per output word + 4 per permutation word) over its time.
  copy       hipMemcpyAsync device to device of 4 x 7 x 2^log_out bytes, then a wait for the device.
  ingest     bfhip_columns_from_rows of the first S rows, same layout, same columns.
  numpy      row-major only, one call per window, 2 windows after a warm-up: bfhip_download of the table, the mask and / or lexsort, one
             fancy-indexed gather, per column the storage-order index and bfhip_upload into a fresh buffer, free.
  time       ms per call: select, copy and ingest alternate in windows, `rounds` rounds (at least five) after a warm-up round (ratelib).
  check      before the timing: the device's columns equal the numpy route's, byte for byte.

No threshold is attached. A run without a GPU fails: nothing here is measured on the host alone."""
import argparse
import ctypes
import statistics

import numpy as np

from ratelib import alternate, cell, emit, events, load_package, require_gpu

import columns_model as model      # tests/ (ratelib put it on the path)

P = (1 << 31) - 1
D2D = 3      # hipMemcpyDeviceToDevice
N_COLS = 7
SELECTIONS = {"filter 1/8": dict(where=[(0, "==", 3)]), "sort by 2 keys": dict(order_by=(1, 2)), "filter 1/8 + sort": dict(where=[(0, "==", 3)], order_by=(1, 2))}


def make_table(log_n):
    rng = np.random.default_rng(log_n)
    n = 1 << log_n
    t = rng.integers(0, P, size=(n, N_COLS), dtype=np.uint32)
    t[:, 0] = rng.permutation(np.tile(np.arange(8, dtype=np.uint32), n // 8))
    t[:, 1] = rng.integers(0, 1024, size=n)
    return t


def measure(pkg, ctx, bare, hip, a, table, src, layout, what, sel):
    n = table.shape[0]
    S = n // 8 if "where" in sel else n
    log_out = max(1, (S - 1).bit_length())
    m = 1 << log_out
    index = model.rows_of_cells(log_out)
    ptrs = []
    try:
        cols = [ctx.malloc(4 * m) for _ in range(N_COLS)]; ptrs += cols
        copy_src, copy_dst = ctx.malloc(4 * m * N_COLS), ctx.malloc(4 * m * N_COLS); ptrs += [copy_src, copy_dst]
        first = pkg.DeviceRows(src.ptr, S, N_COLS, N_COLS) if layout == "rows" else pkg.DeviceRowColumns(src.ptrs, S)

        def select():
            select.last = ctx.rows_select(src, log_out, out=cols, **sel).n_selected

        def select_bare():      # on the second context: alternate() synchronises only ctx around a window, which is enough because the
            # call returns behind its own blocking read-back and the wait of its call-scoped memory
            bare.rows_select(src, log_out, out=cols, **sel)

        def copy():
            assert hip.hipMemcpyAsync(ctypes.c_void_p(copy_dst), ctypes.c_void_p(copy_src), ctypes.c_size_t(4 * m * N_COLS), D2D, None) == 0
            assert hip.hipDeviceSynchronize() == 0

        def ingest():
            ctx.columns_from_rows(first, log_out, out=cols)

        def numpy_route():
            t = ctx.download(table_d, n * N_COLS).reshape(n, N_COLS)
            order = np.flatnonzero(t[:, 0] == 3) if "where" in sel else np.arange(n)
            if "order_by" in sel:
                order = order[np.lexsort((t[order, 2], t[order, 1]))]
            full = np.zeros((m, N_COLS), dtype=np.uint32)
            full[:len(order)] = t[order]
            numpy_route.last = [np.ascontiguousarray(full[:, c][index]) for c in range(N_COLS)]
            for c in numpy_route.last:
                ctx.free(ctx.upload(c))

        select()
        ms = alternate(ctx, {"select": select, "select, no reserve": select_bare, "copy": copy, "ingest": ingest}, a.passes, a.rounds)
        ev = events(ctx, select, a.passes)
        if layout == "rows":
            table_d = src.ptr
            select()
            got = np.stack([ctx.download(p, m) for p in cols])
            numpy_route()
            if select.last != S or got.tobytes() != np.stack(numpy_route.last).tobytes():
                raise SystemExit("rows_select_rate: the device and the numpy route disagree at 2^%d, %s" % (n.bit_length() - 1, what))
            ms.update(alternate(ctx, {"numpy": numpy_route}, 1, 2))
        return ms, ev, log_out
    finally:
        for p in ptrs:
            ctx.free(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=5); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--small", action="store_true"); ap.add_argument("--out")
    ap.add_argument("--reserve-mib", type=int, default=1536)
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("rows_select_rate: at least five rounds")
    pkg = load_package()
    require_gpu(pkg, "rows_select_rate")
    hip = ctypes.CDLL("libamdhip64.so")
    ctx, bare = pkg.Context(0, max_log_domain=16), pkg.Context(0, max_log_domain=16)
    ctx.set_scratch_reserve(a.reserve_mib << 20)
    logs = (14, 16) if a.small else (20, 24)
    lines = [f"bfhip_rows_select (select) of 2^{logs[0]} and 2^{logs[1]} rows x {N_COLS} resident in HBM, all {N_COLS} columns written into the smallest domain that holds the selection, "
             f"beside a device-to-device copy of the output's bytes (copy), bfhip_columns_from_rows of as many unpermuted rows (ingest) and download + numpy + upload "
             f"(numpy, row-major only); select runs on a context with a scratch reserve, `select, no reserve` on one without: {a.rounds} alternating rounds of {a.passes} calls (numpy: 2 rounds of 1 call) after a warm-up round, the context synchronised "
             f"around every window; equal bytes (device = numpy route) checked for the row-major cases. Split by HIP events in one further window: flags = "
             f"k_select_flags (flags and scan), sort = rows_select_sort (key gathers and radix sorts), gather = k_select_gather with GB/s over its algorithmic bytes.", "",
             "case | path | ms per call: median (min-max)"]
    try:
        for log_n in logs:
            table = make_table(log_n)
            n = 1 << log_n
            for layout in ("rows", "columns"):
                held = [ctx.upload(table)] if layout == "rows" else [ctx.upload(table[:, c]) for c in range(N_COLS)]
                src = pkg.DeviceRows(held[0], n, N_COLS, N_COLS) if layout == "rows" else pkg.DeviceRowColumns(held, n)
                try:
                    for what, sel in SELECTIONS.items():
                        ms, ev, log_out = measure(pkg, ctx, bare, hip, a, table, src, layout, what, sel)
                        med = {k: statistics.median(v) for k, v in ms.items()}
                        name = "2^%d x %d %s, %s -> 2^%d" % (log_n, N_COLS, "row-major" if layout == "rows" else "column-major", what, log_out)
                        for path in ("select", "select, no reserve", "copy", "ingest", "numpy"):
                            if path in ms:
                                lines.append(f"{name} | {path} | {cell(ms[path], 4)}")
                        flags, sort, gather = (ev.get(k, (0.0, 0))[0] for k in ("k_select_flags", "rows_select_sort", "k_select_gather"))
                        gather_bytes = (8.0 * N_COLS + 4.0) * (1 << log_out)
                        lines.append(f"{name} | by HIP events, ms per call | flags {flags:.4f}, sort {sort:.4f}, gather {gather:.4f} ({gather_bytes / gather / 1e6:.0f} GB/s)")
                        ratios = f"select / copy {med['select'] / med['copy']:.2f}x; select / ingest {med['select'] / med['ingest']:.2f}x; gather alone / copy {gather / med['copy']:.2f}x"
                        if "numpy" in med:
                            ratios += f"; numpy / select {med['numpy'] / med['select']:.0f}x"
                        lines += [f"{name} | ratios of median ms | {ratios}", ""]
                finally:
                    for p in held:
                        ctx.free(p)
        stats = ctx.scratch_stats()
        lines.append(f"scratch reserve {stats['reserve'] >> 20} MiB, high water {stats['high_water'] / 2**20:.0f} MiB, device allocations by call-scoped memory on that context: {stats['device_allocations']}")
    finally:
        ctx.close(); bare.close()
    emit("\n".join(lines), a.out)


if __name__ == "__main__":
    main()
