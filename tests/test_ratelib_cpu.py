"""tools/ratelib.py, the one timing scheme of the *_rate.py scripts, against a context that only logs what it is asked: the order of
synchronisations, calls and profiler switches IS the scheme. And every converted script: --help works, and without a GPU it says so."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import ratelib  # noqa: E402

SCRIPTS = ("air_check_rate", "air_compiled_rate", "air_compose_rate", "air_program_rate", "air_prove_rate", "grind_poseidon_rate", "logup_batch_rate",
           "logup_program_rate", "pcs_session_rate", "preflight_rate", "relation_multiplicities_rate", "relation_program_rate", "relations_rate",
           "trace_check_rate")

REPORT = {"k_a": {"calls": 12, "total_ms": 3.0, "bytes": 0}, "k_b": {"calls": 4, "total_ms": 1.0, "bytes": 64}, "streams": 4, "note": {"text": "no scope"}}


@pytest.fixture
def fake(pkg):
    """A context that logs; its profiling() is the mirror's own Context.profiling, run over the logging methods."""
    class Fake:
        profiling = pkg.Context.profiling

        def __init__(self):
            self.log = []

        def sync(self):
            self.log.append("sync")

        def profile_enable(self, mode=1):
            self.log.append(("enable", mode))

        def profile_reset(self):
            self.log.append("reset")

        def profile_report(self):
            self.log.append("report")
            return REPORT

        def path(self, name):
            return lambda: self.log.append(name)

    return Fake()


def test_alternate_is_a_warm_up_round_then_rounds_of_synchronised_windows(fake):
    n, rounds = 3, 4
    ms = ratelib.alternate(fake, {"b": fake.path("b"), "a": fake.path("a")}, n, rounds)
    one_round = ["sync"] + ["b"] * n + ["sync"] + ["sync"] + ["a"] * n + ["sync"]
    assert fake.log == one_round * (rounds + 1)
    assert list(ms) == ["b", "a"] and all(len(v) == rounds and all(t >= 0 for t in v) for v in ms.values())


def test_alternate_drops_the_first_round_and_keeps_the_order_measured(fake, monkeypatch):
    readings = iter(range(100))
    monkeypatch.setattr(ratelib, "window", lambda ctx, call, n: float(next(readings)))
    ms = ratelib.alternate(fake, {"x": None, "y": None}, 7, 3)
    assert ms == {"x": [2.0, 4.0, 6.0], "y": [3.0, 5.0, 7.0]}


def test_events_profiles_one_window_and_divides_by_n(fake):
    got = ratelib.events(fake, fake.path("c"), 4)
    assert fake.log == [("enable", 1), "reset", "sync", "c", "c", "c", "c", "sync", "report", ("enable", 0)]
    assert got == {"k_a": (0.75, 3.0), "k_b": (0.25, 1.0)}      # "streams" and "note" are no scope records


def test_events_leaves_the_profiler_off_when_the_call_raises(fake):
    def call():
        fake.log.append("c")
        raise RuntimeError("boom")
    with pytest.raises(RuntimeError, match="boom"):
        ratelib.events(fake, call, 4)
    assert fake.log == [("enable", 1), "reset", "sync", "c", ("enable", 0)]


def test_repeated_resets_before_every_call_and_drops_the_warm_ups(fake):
    kept = ratelib.repeated(fake, fake.path("c"), 2, 3)
    assert fake.log == [("enable", 1), "reset"] + ["reset", "c", "report"] * 5 + [("enable", 0)]
    assert len(kept) == 2
    for wall, gpu in kept:
        assert wall >= 0 and gpu == {"k_a": 3.0, "k_b": 1.0}


def test_cell_text():
    xs = [0.04912, 0.04871, 0.04874, 0.04869, 0.04905]
    assert ratelib.cell(xs, 4) == "0.0487 (0.0487-0.0491)"
    assert ratelib.cell(xs, 3) == "0.049 (0.049-0.049)"


def test_emit_replaces_and_appends(tmp_path, capsys):
    out = tmp_path / "table.txt"
    ratelib.emit("one\n", str(out))
    ratelib.emit("two\n", str(out))
    assert out.read_text() == "two\n"
    ratelib.emit("three\n", str(out), append=True)
    assert out.read_text() == "two\nthree\n"
    ratelib.emit("four\n", None)
    assert capsys.readouterr().out == "one\ntwo\nthree\nfour\n"


def test_require_gpu():
    class Pkg:
        def __init__(self, n):
            self.n = n

        def device_count(self):
            return self.n

    ratelib.require_gpu(Pkg(1), "some_rate")
    with pytest.raises(SystemExit) as e:
        ratelib.require_gpu(Pkg(0), "some_rate")
    assert str(e.value) == "some_rate: no GPU"


def _run(script, *args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")      # no device for the child, also where the machine has one
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", script + ".py"), *args], capture_output=True, text=True, timeout=120, env=env)


@pytest.mark.parametrize("script", SCRIPTS)
def test_script_help(pkg, script):
    r = _run(script, "--help")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "usage:" in r.stdout


@pytest.mark.parametrize("script", SCRIPTS)
def test_script_without_a_gpu_says_so(pkg, script):
    r = _run(script)
    assert r.returncode != 0
    assert r.stderr.strip().splitlines()[-1] == script + ": no GPU", r.stderr[-2000:]
    assert "Traceback" not in r.stderr
