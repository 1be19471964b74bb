"""A plain-Python restatement of the SHAPE decisions of fft_plan (stwo-brainfuck_amd/csrc/fft_plan.h) for one job = the columns of one size:
which kernel runs each pass, over which layers, how many columns one workgroup walks and how many workgroups the launch has. It exists to
choose and to label test cases (tests/test_fft_plan_model_cpu.py holds every case of tests/test_gpu_fft.py and
tests/test_gpu_pcs_commit_large.py to the property it is named for). It is never the reference of a value: values are compared with the CPU oracle.

tests/test_fft_plan_cpu.py holds the model to the planner: it compiles fft_plan.h into a stand-alone program (tests/native/fft_plan_host.cpp) and
compares every pass of 11 136 single-job plans, and the constants below, with what the header itself computes. One GPU test
(tests/test_gpu_fft.py::test_library_launches_what_the_plan_model_says) holds it to the workgroup totals the library launches.

A job is (inverse, log, src_log, ncols) as api_ops.hip builds it: interpolate(log) = (True, log, log, n), evaluate(log -> log_eval) =
(False, log_eval, log, n). Row-granular ("replicated") columns are the same job 4 levels lower in line mode, which changes no shape.

Rules restated (fft_plan.h):
  fft_layers          nl, the layers that run: all of them inverse; forward the source's (the layers above only duplicate), at least 2 past 32 cells
  fft_passes_tiny     log <= FFT_TINY_MAX_LOG: k_fft_tiny, 256 >> log columns per workgroup, no column loop
  fft_passes_fast     log >= TILE_LOG and nl >= FFT_FAST_MIN_LAYERS: ns strided passes of 7 layers behind a contiguous pass of k0 = nl - 7 ns in [6, 12];
                      FFT_TWO_PASS_MIN_LAYERS <= nl <= FFT_TWO_PASS_MAX_LAYERS (BFHIP_FFT_TWO_PASS unset): ONE strided pass of nl - 12 layers behind k0 = 12.
                      ntiles = 2^(log - 12); cols_per_block starts at ncols and halves, rounding up, while cpb > 1 and ntiles * ceil(ncols / cpb) <
                      FFT_MIN_BLOCKS; gy = ceil(ncols / cpb). k_fft_tile12: grid_x = ntiles. k_fft_stridedK<K>: rows of 2^cl cells, cl =
                      FFT_STRIDED_K10_CHUNK_LOG at K = 10 and FFT_STRIDED_K_CHUNK_LOG otherwise; grid_x = 2^(log - K - cl). k_fft_strided7: lo = k0 + 7 (p - 1);
                      wide (256-byte rows) when lo >= 6 and log >= FFT_STRIDED_WIDE_MIN_LOG: grid_x = ntiles / 2, else ntiles
  fft_passes_generic  everything else (k_fft_pass): a contiguous pass of min(nl, min(log, 12)) layers, strided passes of balanced length <= 7 in tiles of
                      2^(k + 5) cells; cols_per_block doubles from 1 while ntiles * ceil(ncols / cpb) > FFT_MAX_BLOCKS_GENERIC and cpb < ncols
  fft_plan            execution order: inverse = contiguous pass first, forward = mirrored; a launch has grid_x * gy workgroups per group (tiny: grid_x);
                      single-pass transforms below 2^12 cells and tiny ones ride in the plan's first k_fft_tile12 launch when it has one"""
from collections import Counter, namedtuple

TILE_LOG, CHUNK_LOG, STRIDED_K, WIDE_MIN_LOG, MIN_BLOCKS, MAX_BLOCKS_GENERIC = 12, 5, 7, 20, 2048, 8192
TINY_MAX_LOG, FAST_MIN_LAYERS, TWO_PASS_MIN_LAYERS, TWO_PASS_MAX_LAYERS, STRIDED_K_CHUNK_LOG, STRIDED_K10_CHUNK_LOG = 5, 6, 20, 22, 5, 4

# kind: "tile12" | "strided7_narrow" | "strided7_wide" | "stridedK8" | "stridedK9" | "stridedK10" | "pass" | "tiny"; lo, k: the layers [lo, lo + k)
Pass = namedtuple("Pass", "kind lo k cols_per_block grid_x gy workgroups")

# the name the profiler gives a launch of the kind (fft_run); k_fft_tiny is launched without a record
KERNEL = {"tile12": "k_fft_tile12", "strided7_narrow": "k_fft_strided7", "strided7_wide": "k_fft_strided7", "stridedK8": "k_fft_stridedK",
          "stridedK9": "k_fft_stridedK", "stridedK10": "k_fft_stridedK", "pass": "k_fft_pass", "tiny": None}


def _ceil_div(a, b):
    return (a + b - 1) // b


def plan(inverse, log, src_log, ncols):
    """The passes of the job in execution order."""
    assert ncols >= 1 and src_log <= log
    nl = log if inverse else (2 if log > TINY_MAX_LOG and src_log < 2 else src_log)
    if log <= TINY_MAX_LOG:
        gx = _ceil_div(ncols, 256 >> log)
        return [Pass("tiny", 0, nl, 1, gx, 1, gx)]
    out = []
    if log >= TILE_LOG and nl >= FAST_MIN_LAYERS:
        ns = (nl - 12 + 6) // 7 if nl > 12 else 0
        k0 = nl - 7 * ns
        big_k = nl - 12 if TWO_PASS_MIN_LAYERS <= nl <= TWO_PASS_MAX_LAYERS else 0
        if big_k:
            ns, k0 = 1, 12
        np_ = 1 + ns
        ntiles = 1 << (log - 12)
        cpb = ncols
        while cpb > 1 and ntiles * _ceil_div(ncols, cpb) < MIN_BLOCKS:
            cpb = (cpb + 1) // 2
        gy = _ceil_div(ncols, cpb)
        for pi in range(np_):
            p = pi if inverse else np_ - 1 - pi
            if p == 0:
                kind, lo, k, gx = "tile12", 0, k0, ntiles
            elif big_k:
                cl = STRIDED_K10_CHUNK_LOG if big_k == 10 else STRIDED_K_CHUNK_LOG
                kind, lo, k, gx = "stridedK%d" % big_k, 12, big_k, 1 << (log - big_k - cl)
            else:
                lo = k0 + 7 * (p - 1)
                wide = lo >= 6 and log >= WIDE_MIN_LOG
                kind, k, gx = ("strided7_wide" if wide else "strided7_narrow"), 7, (ntiles // 2 if wide else ntiles)
            out.append(Pass(kind, lo, k, cpb, gx, gy, gx * gy))
        return out
    tile_log = min(log, TILE_LOG)
    bounds = [0, min(nl, tile_log)]
    while bounds[-1] < nl:
        rem = nl - bounds[-1]
        left = _ceil_div(rem, STRIDED_K)
        bounds.append(bounds[-1] + _ceil_div(rem, left))
    np_ = len(bounds) - 1
    for pi in range(np_):
        p = pi if inverse else np_ - 1 - pi
        lo, k = bounds[p], bounds[p + 1] - bounds[p]
        ntiles = 1 << (log - (tile_log if lo == 0 else k + CHUNK_LOG))
        cpb = 1
        while ntiles * _ceil_div(ncols, cpb) > MAX_BLOCKS_GENERIC and cpb < ncols:
            cpb *= 2
        gy = _ceil_div(ncols, cpb)
        out.append(Pass("pass", lo, k, cpb, ntiles, gy, ntiles * gy))
    return out


def interpolate(log, ncols):
    return plan(True, log, log, ncols)


def evaluate(log, log_eval, ncols):
    return plan(False, log_eval, log, ncols)


def kinds(passes):
    return [p.kind for p in passes]


def ragged(p, ncols):
    """The last column block of a workgroup row is shorter than the others."""
    return p.cols_per_block >= 2 and ncols % p.cols_per_block != 0


def launch_names(inverse, passes):
    """What Context.profile_report lists for the job run alone under BFHIP_FFT_PROF_DETAIL=1: {"<kernel><inverse>/b<workgroups>/g1": calls}."""
    tag = "<true>" if inverse else "<false>"
    return dict(Counter("%s%s/b%d/g1" % (KERNEL[p.kind], tag, p.workgroups) for p in passes if KERNEL[p.kind]))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# test_many_columns_per_workgroup: (trace log, columns) -> what the inverse transform and the forward one to log + 1 are there for.
# kinds in execution order; cpb = cols_per_block of every pass; "all" = one workgroup row walks every column
MANY_COLUMNS = {
    (18, 65): dict(inverse=dict(kinds=["tile12", "strided7_narrow"], k0=11, cpb=2, ragged=True),
                   forward=dict(kinds=["strided7_narrow", "tile12"], k0=11, cpb=3, ragged=True)),
    (19, 17): dict(inverse=dict(kinds=["tile12", "strided7_narrow"], k0=12, cpb=1, ragged=False),          # the control: no column loop
                   forward=dict(kinds=["strided7_wide", "tile12"], k0=12, cpb=2, ragged=True)),
    (20, 17): dict(inverse=dict(kinds=["tile12", "stridedK8"], k0=12, cpb=2, ragged=True),
                   forward=dict(kinds=["stridedK8", "tile12"], k0=12, cpb=5, ragged=True)),
    (21, 9): dict(inverse=dict(kinds=["tile12", "stridedK9"], k0=12, cpb=2, ragged=True),
                  forward=dict(kinds=["stridedK9", "tile12"], k0=12, cpb=5, ragged=True)),
    (22, 5): dict(inverse=dict(kinds=["tile12", "stridedK10"], k0=12, cpb=3, ragged=True),
                  forward=dict(kinds=["stridedK10", "tile12"], k0=12, cpb=5, ragged=False, all=True)),
    (23, 2): dict(inverse=dict(kinds=["tile12", "strided7_wide", "strided7_wide"], k0=9, cpb=2, ragged=False, all=True),
                  forward=dict(kinds=["strided7_wide", "strided7_wide", "tile12"], k0=9, cpb=2, ragged=False, all=True)),
}
# test_many_columns_under_larger_blowups: (log, log_eval, columns) -> the forward transform
LARGER_BLOWUPS = {
    (16, 20, 17): dict(kinds=["strided7_wide", "tile12"], k0=9, cpb=2, ragged=True),
    (18, 22, 5): dict(kinds=["strided7_wide", "tile12"], k0=11, cpb=3, ragged=True),
}
BETWEEN_SIZES = (15, 17, 18)          # test_sizes_between_the_visited_ones, 3 columns: k0 = 8, 10, 11 in front of one narrow strided pass
BETWEEN_COLUMNS = 3
TINY_LOGS = (3, 4, 5)                 # test_tiny_transforms_over_several_workgroups


def tiny_column_counts(log):
    per = 256 >> log
    return (per + 1, 3 * per - 1)      # two and three workgroups, the last one partial


# tests/test_gpu_pcs_commit_large.py: session -> (log_blowup_factor, top LDE level, columns of the largest size class). The largest class of b1, b2
# and b4 is 2^19, 2^19 and 2^18 rows: its forward transform walks 2, 2 and 3 columns per workgroup with a shorter last block (wide strided7), its
# inverse one column. No trace of 2^19 rows or fewer runs 20 layers, so none of the three reaches k_fft_stridedK; b1_top22 (2^21 rows) does, in both
# directions, with 2 and 5 columns per workgroup.
SESSIONS = {"b1": (1, 20, 17), "b2": (2, 21, 9), "b4": (4, 22, 5), "b1_top22": (1, 22, 9)}


def session_kernels(log_blowup, tree_logs, forms):
    """The kernel names Context.profile_report lists after the commits of a session (BFHIP_FFT_PROF_DETAIL unset): a tree of evaluations
    (form 0) is one inverse plan over its size classes, every tree one forward plan to log + log_blowup. Single-pass transforms below 2^12
    cells and tiny ones ride in the plan's first k_fft_tile12 launch when it has one (fft_plan.h: fft_plan) and leave no name of their own."""
    names = set()
    for logs, form in zip(tree_logs, forms):
        plans = [(False, [plan(False, log + log_blowup, log, logs.count(log)) for log in sorted(set(logs))])]
        if form == 0:
            plans.append((True, [plan(True, log, log, logs.count(log)) for log in sorted(set(logs))]))
        for inverse, jobs in plans:
            host = any(p.kind == "tile12" for job in jobs for p in job)
            for job in jobs:
                guest = host and len(job) == 1 and job[0].kind in ("pass", "tiny") and job[0].lo == 0
                names |= {KERNEL[p.kind] + ("<true>" if inverse else "<false>") for p in job if KERNEL[p.kind] and not guest}
    return names
