"""CPU: the FFT planner itself (csrc/fft_plan.h: host only, plain C++), compiled into the stand-alone program tests/native/fft_plan_host.cpp under
g++ -fsanitize=address,undefined and run once, directly. The program prints the planner's constants, one line per plan of a single-job grid (inverse
at log 0..28, forward at every src_log <= log <= 28, 24 column counts; the four knob settings, and line mode) and 56 multi-job plans; this module
holds tests/fft_plan_model.py to those lines, checks the knobs and the packing of launches, and pins the whole output by its sha256.

PARENT_SHA256 was recorded from the planner as it stood inside fft.hip before it became a header: the same program built against that text
(its fft_plan function, the structs of kernels.h, the kind enum and the constants, compiled as plain C++; the two function-local environment
switches replaced by the knobs parameter so that one process prints all four settings). A refactor of fft_plan.h that changes any field a kernel
reads, any launch or any accounting figure changes the hash; so does a deliberate change of plan, which then records a new one."""
import hashlib
import os
import re
import subprocess

import pytest

import fft_plan_model as fm
import test_gpu_pcs_commit_large as large
from conftest import ROOT

PARENT_SHA256 = "2581e2015f3dd2cac290d1bd93a82bc2af502aa9546a5b10f3b9ca28bc9096bb"
KIND = ["tile12", "strided7_narrow", "strided7_wide", "pass", "tiny", "stridedK8", "stridedK9", "stridedK10"]      # the kind enum of fft_plan.h
COUNTS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 999, 1000)
NOHOST = [(3, 2), (5, 70), (7, 1), (9, 3), (10, 40)]      # (log, columns) of the batch without a job of 2^12 cells


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fft_plan") / "fft_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "fft_plan_host.cpp")])
    r = subprocess.run([exe], capture_output=True, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (r.returncode, err[-2000:])
    return r.stdout


def _fields(text):
    return {k: v for k, v in (f.split("=", 1) for f in text.split())}


def _parse(line):
    """-> (header fields, [(launch fields, [group fields])]); numbers stay strings except where a check reads them."""
    parts = line.split(" | ")
    launches = []
    for p in parts[1:]:
        chunks = p.split(" ; ")
        launches.append((_fields(chunks[0]), [_fields(c) for c in chunks[1:]]))
    head = _fields(parts[0][2:])
    head["jobs"] = [tuple(int(x) for x in j.split(":")) for j in head["jobs"].split(",")]      # (log, src_log, ncols, circle)
    return head, launches


@pytest.fixture(scope="module")
def lines(output):
    text = output.decode().splitlines()
    assert text[0].startswith("C ") and all(l[:2] in ("S ", "M ") for l in text[1:])
    return text


def _kernel_kind(launch, group):
    return int(group["gkind"]) or int(launch["kind"])


def _gy(launch, group):
    return 1 if _kernel_kind(launch, group) == KIND.index("tiny") else -(-int(group["ncols"]) // int(group["cpb"]))


def _passes_of(launches, job):
    """The passes of one job in launch order, as the model's tuples; workgroups = grid_x * gy."""
    out = []
    for L, groups in launches:
        for g in groups:
            if int(g["job"]) == job:
                kind = KIND[_kernel_kind(L, g)]
                assert ("cpb" in g) == (kind != "tiny") and ("tile_log" in g) == (kind in ("tile12", "pass") and g["lo"] == "0")
                out.append((kind, int(g["lo"]), int(g["k"]), int(g.get("cpb", 1)), int(g["grid_x"]), int(g["grid_x"]) * _gy(L, g)))
    return out


def _model(inverse, job):
    log, src_log, ncols, _ = job
    return [(p.kind, p.lo, p.k, p.cols_per_block, p.grid_x, p.workgroups) for p in fm.plan(inverse, log, src_log, ncols)]


def test_constants_are_those_of_the_planner(lines):
    """The numbers the model restates, as the compiled header prints them: a changed threshold makes the model stale, and says so here."""
    c = {k: int(v) for k, v in _fields(lines[0][2:]).items()}
    assert c["TILE_LOG"] == fm.TILE_LOG and c["CHUNK_LOG"] == fm.CHUNK_LOG and c["STRIDED_K"] == fm.STRIDED_K == fm.TILE_LOG - fm.CHUNK_LOG
    assert c["WIDE_MIN_LOG"] == fm.WIDE_MIN_LOG and c["MIN_BLOCKS"] == fm.MIN_BLOCKS and c["MAX_BLOCKS_GENERIC"] == fm.MAX_BLOCKS_GENERIC
    assert (c["TWO_PASS_MIN_LAYERS"], c["TWO_PASS_MAX_LAYERS"]) == (fm.TWO_PASS_MIN_LAYERS, fm.TWO_PASS_MAX_LAYERS)
    assert (c["STRIDED_K_CHUNK_LOG"], c["STRIDED_K10_CHUNK_LOG"]) == (fm.STRIDED_K_CHUNK_LOG, fm.STRIDED_K10_CHUNK_LOG)
    assert (c["TINY_MAX_LOG"], c["FAST_MIN_LAYERS"]) == (fm.TINY_MAX_LOG, fm.FAST_MIN_LAYERS)
    assert c["K_KINDS"] == len(KIND) and lines[0].split("kinds=")[1].split()[0] == "01234567" and c["sizeof_PassArgs"] == 80


def test_single_job_plans_are_what_the_model_says(lines):
    """Every single-job line under the default knobs, circle and line mode: the same (kind, lo, k, cols_per_block, grid_x, workgroups) per pass in
    execution order, no exclusions (k_fft_tiny reads no cols_per_block and the program prints none: the other five)."""
    grid = [(inv, log, src_log, n) for inv in (1, 0) for log in range(29) for src_log in (range(log + 1) if not inv else [log]) for n in COUNTS]
    assert len(grid) == 464 * len(COUNTS) == 11136
    seen = {0: [], 1: []}
    mismatches = []
    for line in lines:
        if not line.startswith("S knobs=11 "):
            continue
        head, launches = _parse(line)
        (job,) = head["jobs"]
        inv = int(head["inv"])
        seen[job[3]].append((inv, job[0], job[1], job[2]))
        assert all(L["ngroups"] == "1" and g["block0"] == "0" and g["gkind"] == "0" for L, (g,) in launches)
        got = _passes_of(launches, 0)
        assert [w for *_, w in got] == [int(L["total_blocks"]) for L, _ in launches]
        if got != _model(bool(inv), job):
            mismatches.append((line[:60], got, _model(bool(inv), job)))
    assert seen[1] == grid and seen[0] == grid          # circle mode and line mode, in the program's order
    assert not mismatches, (len(mismatches), mismatches[:3])


def test_the_grid_straddles_every_threshold(lines):
    """Both sides of every rule, among the default-knob lines themselves: the path by log and nl, k0's range, the wide rows, the two-pass window, and
    a column count on either side of each cols_per_block rule at more than one size."""
    by_job = {}
    for line in lines:
        if line.startswith("S knobs=11 ") and line.split("jobs=")[1].split()[0].endswith(":1"):
            head, launches = _parse(line)
            by_job[(int(head["inv"]),) + head["jobs"][0][:3]] = _passes_of(launches, 0)
    kinds = lambda *job: [p[0] for p in by_job[job]]
    assert kinds(1, 5, 5, 1) == ["tiny"] and kinds(1, 6, 6, 1) == ["pass"] and kinds(1, 11, 11, 1) == ["pass"] and kinds(1, 12, 12, 1) == ["tile12"]
    assert kinds(0, 12, 5, 1) == ["pass"] and kinds(0, 12, 6, 1) == ["tile12"]                                             # nl 5|6
    assert kinds(1, 12, 12, 1) == ["tile12"] and kinds(1, 13, 13, 1) == ["tile12", "strided7_narrow"]                      # nl 12|13
    assert kinds(1, 19, 19, 1) == ["tile12", "strided7_narrow"] and kinds(1, 20, 20, 1) == ["tile12", "stridedK8"]         # nl and log 19|20
    assert kinds(1, 22, 22, 1) == ["tile12", "stridedK10"] and kinds(1, 23, 23, 1) == ["tile12", "strided7_wide", "strided7_wide"]      # nl 22|23
    assert kinds(0, 19, 18, 1) == ["strided7_narrow", "tile12"] and kinds(0, 20, 18, 1) == ["strided7_wide", "tile12"]     # log 19|20 at the same layers
    # the wide rows need lo >= 6, and no strided pass of the fast path starts lower (k0 >= 6): its lowest start, lo = 6, on both sides of log 19|20
    assert [p[:2] for p in by_job[(0, 19, 13, 1)]] == [("strided7_narrow", 6), ("tile12", 0)] and [p[:2] for p in by_job[(0, 20, 13, 1)]] == [("strided7_wide", 6), ("tile12", 0)]
    assert min(p[1] for passes in by_job.values() for p in passes if p[0].startswith("strided")) == 6
    # the 2048 rule: ntiles * ceil(ncols / cpb) on either side, at three sizes; the 8192 rule likewise
    for log, below, above in ((16, 129, 255), (18, 33, 64), (20, 9, 16), (22, 2, 3)):
        assert by_job[(1, log, log, below)][0][3] == 1 and by_job[(1, log, log, above)][0][3] == 2, log
    for log, below, above in ((20, 32, 33), (21, 16, 17), (23, 4, 5)):
        assert by_job[(0, log, 2, below)][0][3] == 1 and by_job[(0, log, 2, above)][0][3] == 2, log


def test_the_knobs(lines):
    """two_pass off: no k_fft_stridedK, the 20..22-layer jobs run tile12 + two strided passes of 7 layers. fuse_small off: no guest groups."""
    kinds_of = lambda line: [int(k) for k in re.findall(r"\| kind=(\d+)", line)]
    guests = {"11": 0, "01": 0, "10": 0, "00": 0}
    fell_back = 0
    for line in lines[1:]:
        knobs = line.split("knobs=")[1][:2]
        guests[knobs] += len(re.findall(r" gkind=[1-9]", line))
        if knobs[0] == "0":
            assert not any(KIND[k].startswith("stridedK") for k in kinds_of(line)), line[:80]
            if line.startswith("S "):
                head, launches = _parse(line)
                (job,) = head["jobs"]
                inv = int(head["inv"])
                if any(p[0].startswith("stridedK") for p in _model(bool(inv), job)):
                    nl = sum(p[2] for p in _model(bool(inv), job))
                    got = _passes_of(launches, 0)[::1 if inv else -1]
                    assert fm.TWO_PASS_MIN_LAYERS <= nl <= fm.TWO_PASS_MAX_LAYERS
                    assert [(p[0].split("_")[0], p[1], p[2]) for p in got] == [("tile12", 0, nl - 14), ("strided7", nl - 14, 7), ("strided7", nl - 7, 7)], line[:80]
                    fell_back += 1
    assert guests["10"] == guests["00"] == 0 and guests["11"] == guests["01"] > 0
    n_two_pass = sum(1 for line in lines if line.startswith("S knobs=11 ") and line.split("jobs=")[1].split()[0].endswith(":1") and re.search(r"\| kind=[567] ", line))
    assert fell_back == 2 * n_two_pass > 0          # the settings 01 and 00 each visit the grid once, in circle mode

def _multi(lines):
    return [_parse(l) for l in lines if l.startswith("M ")]


def test_multi_job_plans_pack_every_pass_once(lines):
    plans = _multi(lines)
    assert len(plans) == 4 * (4 * 3 + 2)
    for head, launches in plans:
        inv = bool(int(head["inv"]))
        # within each launch the groups' workgroup ranges tile [0, total_blocks) in order
        for L, groups in launches:
            assert int(L["ngroups"]) == len(groups) >= 1
            at = 0
            for g in groups:
                assert int(g["block0"]) == at, (head, L)
                at += int(g["grid_x"]) * _gy(L, g)
            assert at == int(L["total_blocks"]), (head, L)
        # every job's passes exactly once, in layer order: inverse upward from layer 0, forward down to it
        for j, job in enumerate(head["jobs"]):
            got = _passes_of(launches, j)
            layers = got if inv else got[::-1]
            assert layers[0][1] == 0 and all(b[1] == a[1] + a[2] for a, b in zip(layers, layers[1:])), (head, j)
            nl = job[0] if inv else (2 if job[0] > 5 and job[1] < 2 else job[1])
            assert layers[-1][1] + layers[-1][2] == nl, (head, j)
            if head["knobs"][0] == "1":
                assert got == _model(inv, job), (head, j)
        assert sum(len(g) for _, g in launches) == sum(len(_passes_of(launches, j)) for j in range(len(head["jobs"])))
        # guests sit in the earliest k_fft_tile12 launch, and only there; with fuse_small on, every single-pass transform below 2^12 cells does
        hosts = [i for i, (L, _) in enumerate(launches) if L["kind"] == "0"]
        for i, (L, groups) in enumerate(launches):
            for g in groups:
                single = int(g["log"]) < fm.TILE_LOG
                assert (g["gkind"] != "0") == (single and bool(hosts) and head["knobs"][1] == "1"), (head, g)
                if g["gkind"] != "0":
                    assert i == hosts[0] and KIND[int(g["gkind"])] in ("pass", "tiny")
        if head["name"] == "nohost":
            assert not hosts and {L["kind"] for L, _ in launches} == {"3", "4"} and [(j[1], j[2]) for j in head["jobs"]] == NOHOST


def test_session_plans_launch_the_kernels_the_model_names(lines):
    """The multi-job plans are the size classes of the sessions of tests/test_gpu_pcs_commit_large.py, and under the default knobs their launches carry
    the kernel names fft_plan_model.session_kernels() gives."""
    plans = [(h, l) for h, l in _multi(lines) if h["knobs"] == "11" and h["name"] != "nohost"]
    assert [h["name"] for h, _ in plans] == [n for n in fm.SESSIONS for _ in range(3)]
    for name, (b, top, nbig) in fm.SESSIONS.items():
        trees = [[c[0] for c in t] for t in large.session_trees(name)]
        want_jobs = []
        for t, logs in enumerate(trees):
            classes = [(log, logs.count(log)) for log in sorted(set(logs))]
            want_jobs.append((str(t), "0", [(log + b, log, n, 1) for log, n in classes]))
            if large.FORMS[t] == 0:
                want_jobs.append((str(t), "1", [(log, log, n, 1) for log, n in classes]))
        mine = [(h, l) for h, l in plans if h["name"] == name]
        assert [(h["tree"], h["inv"], h["jobs"]) for h, _ in mine] == want_jobs
        names = set()
        for h, launches in mine:
            tag = "<true>" if h["inv"] == "1" else "<false>"
            names |= {fm.KERNEL[KIND[int(L["kind"])]] + tag for L, _ in launches if fm.KERNEL[KIND[int(L["kind"])]]}
        assert names == fm.session_kernels(b, trees, large.FORMS), name


def test_output_is_the_parent_planners(output):
    """Pins what the model does not speak of: src_mask, scale, circle, tw_total, the src / dst choice, block0, guest kinds, the accounting doubles."""
    assert hashlib.sha256(output).hexdigest() == PARENT_SHA256
