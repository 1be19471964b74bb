"""CPU: every case of the many-columns tests of tests/test_gpu_fft.py and of tests/test_gpu_pcs_commit_large.py still has the property it is
named for, by tests/fft_plan_model.py: the kernel kind of every pass, k0, cols_per_block >= 2, a shorter last column block, one block walking
every column. A case that stops reaching its path (a planner threshold moved, a column count changed) fails here instead of passing for
nothing on the GPU. That the model is the library's planner is held elsewhere: tests/test_fft_plan_cpu.py compares it, constants and plans, with
csrc/fft_plan.h compiled into a stand-alone program, and the GPU test test_library_launches_what_the_plan_model_says with what the library launches."""
import pytest

import fft_plan_model as fm
import pcs_generic_cases as gc
import test_gpu_pcs_commit_large as large


def _check(passes, ncols, want, what):
    assert fm.kinds(passes) == want["kinds"], what
    tile = next(p for p in passes if p.kind == "tile12")
    assert tile.k == want["k0"] and tile.lo == 0, what
    assert {p.cols_per_block for p in passes} == {want["cpb"]}, what
    assert all(fm.ragged(p, ncols) == want["ragged"] for p in passes), what
    assert all((p.cols_per_block == ncols and p.gy == 1) == bool(want.get("all")) for p in passes), what
    # the layers of the passes tile the layers that run
    lo = 0
    for p in sorted(passes, key=lambda p: p.lo):
        assert p.lo == lo, what
        lo += p.k
    for p in passes:
        assert p.workgroups == p.grid_x * p.gy and p.gy == -(-ncols // p.cols_per_block), what


@pytest.mark.parametrize("log,ncols", list(fm.MANY_COLUMNS), ids=lambda v: str(v))
def test_many_columns_cases_reach_their_paths(log, ncols):
    want = fm.MANY_COLUMNS[(log, ncols)]
    inv, fwd = fm.interpolate(log, ncols), fm.evaluate(log, log + 1, ncols)
    _check(inv, ncols, want["inverse"], ("inverse", log, ncols))
    _check(fwd, ncols, want["forward"], ("forward", log, ncols))
    assert sum(p.k for p in inv) == log and sum(p.k for p in fwd) == log      # forward: the top layer only duplicates


def test_many_columns_table_covers_what_it_is_there_for():
    """Across the table: cols_per_block 2, 3 and 5; a shorter last block under every kernel with a column loop; the control without one;
    the plan with two strided passes, where 2048 tiles alone make one block walk every column."""
    seen, ragged_kinds = set(), set()
    for (log, ncols) in fm.MANY_COLUMNS:
        for passes in (fm.interpolate(log, ncols), fm.evaluate(log, log + 1, ncols)):
            for p in passes:
                seen.add((p.kind, p.cols_per_block))
                if fm.ragged(p, ncols):
                    ragged_kinds.add(p.kind)
    assert {c for _, c in seen} == {1, 2, 3, 5}
    assert ragged_kinds == {"tile12", "strided7_narrow", "strided7_wide", "stridedK8", "stridedK9", "stridedK10"}
    assert [p.kind for p in fm.interpolate(23, 2)].count("strided7_wide") == 2 and fm.interpolate(23, 2)[0].grid_x == 2048
    assert {p.cols_per_block for p in fm.interpolate(19, 17)} == {1}
    assert list(fm.MANY_COLUMNS) == [(18, 65), (19, 17), (20, 17), (21, 9), (22, 5), (23, 2)]


@pytest.mark.parametrize("log,log_eval,ncols", list(fm.LARGER_BLOWUPS), ids=lambda v: str(v))
def test_larger_blowup_cases_reach_their_paths(log, log_eval, ncols):
    passes = fm.evaluate(log, log_eval, ncols)
    _check(passes, ncols, fm.LARGER_BLOWUPS[(log, log_eval, ncols)], (log, log_eval, ncols))
    assert passes[0].lo == log - 7 and sum(p.k for p in passes) == log


def test_sizes_between_the_visited_ones_have_the_k0_they_are_named_for():
    got = []
    for log in fm.BETWEEN_SIZES:
        inv, fwd = fm.interpolate(log, fm.BETWEEN_COLUMNS), fm.evaluate(log, log + 1, fm.BETWEEN_COLUMNS)
        assert fm.kinds(inv) == ["tile12", "strided7_narrow"] and fm.kinds(fwd) == ["strided7_narrow", "tile12"]
        assert fwd[1].k == inv[0].k
        got.append(inv[0].k)
    assert got == [8, 10, 11]


def test_tiny_cases_fill_two_and_three_workgroups():
    for log in fm.TINY_LOGS:
        per = 256 >> log
        for ncols, groups in zip(fm.tiny_column_counts(log), (2, 3)):
            (p,) = fm.interpolate(log, ncols)
            assert p.kind == "tiny" and p.workgroups == groups and ncols % per != 0 and ncols % (64 >> log) != 0      # a partly filled last wave
            (q,) = fm.evaluate(log, log + 1, ncols)
            assert q.kind == ("tiny" if log < 5 else "pass") and q.k == log


@pytest.mark.parametrize("name", list(fm.SESSIONS))
def test_session_trees_are_what_their_module_says(name):
    b, top, nbig = fm.SESSIONS[name]
    big = top - b
    assert top <= large.MAX_LOG_DOMAIN
    trees = large.session_trees(name)
    assert len(trees) == 2 == len(large.FORMS) and set(large.FORMS) == {0, 1}
    for tree in trees:
        logs = [c[0] for c in tree]
        assert max(logs) == big and logs.count(big) == nbig and len({c[2] for c in tree}) == len(tree)
        small = [l for l in logs if l != big]
        assert any(l in (4, 5) for l in small) and any(6 <= l <= 11 for l in small) and len({l for l in small if 12 <= l <= 19}) >= 2
        assert len(set(small)) >= 4 and len(small) > len(set(small))                       # one size twice
        fams = [c[1] for c in tree]
        assert "zero" in fams and "const" in fams and {f for l, f, _ in tree if l == big} == {"uniform", "max", "edge"}
        assert logs != sorted(logs) and logs != sorted(logs, reverse=True)                 # caller order is no size order
        assert [l for l in logs[:nbig]] != [big] * nbig                                    # the largest class is not one run of the caller's list
        fwd = fm.evaluate(big, top, nbig)
        assert all(p.cols_per_block >= 2 and fm.ragged(p, nbig) for p in fwd), (name, fwd)
    kernels = fm.session_kernels(b, [[c[0] for c in t] for t in trees], large.FORMS)
    both = {"k_fft_tile12<true>", "k_fft_tile12<false>", "k_fft_strided7<true>", "k_fft_strided7<false>"}
    assert both <= kernels
    # k_fft_stridedK needs 20 to 22 layers: a trace of 2^20 rows or more
    assert {k for k in kernels if "stridedK" in k} == ({"k_fft_stridedK<true>", "k_fft_stridedK<false>"} if big >= 20 else set())
    if big >= 20:
        inv = fm.interpolate(big, nbig)
        assert all(p.cols_per_block >= 2 and fm.ragged(p, nbig) for p in inv) and inv[1].kind.startswith("stridedK")


def test_sessions_cover_the_blowups_and_levels():
    assert [fm.SESSIONS[n][:2] for n in ("b1", "b2", "b4")] == [(1, 20), (2, 21), (4, 22)]
    assert [fm.SESSIONS[n][2] for n in ("b1", "b2", "b4")] == [17, 9, 5]
    assert any(fm.SESSIONS[n][1] - fm.SESSIONS[n][0] >= 20 for n in fm.SESSIONS)           # one session runs k_fft_stridedK


def test_wide20_has_a_many_column_class_above_level_18():
    case = gc.BY_NAME["wide20"]
    b = case.cfg["log_blowup_factor"]
    logs = [l for t in case.logs for l in t]
    assert b == 1 and case.max_log + b == 20 == gc.MAX_LOG_DOMAIN and len(case.logs) == 1 and logs.count(19) == 17
    fwd = fm.evaluate(19, 20, 17)
    assert fm.kinds(fwd) == ["strided7_wide", "tile12"] and all(p.cols_per_block == 2 and fm.ragged(p, 17) for p in fwd)
    small = set(logs) - {19}
    assert small & {4, 5} and any(6 <= l <= 11 for l in small) and len({l for l in small if 12 <= l <= 18}) >= 2
    assert len(case.points) == 2 and any(len(c) == 2 for t in case.samples for c in t) and all(c for t in case.samples for c in t)
    assert any(len(c) == 2 for l, c in zip(case.logs[0], case.samples[0]) if l == 19)
