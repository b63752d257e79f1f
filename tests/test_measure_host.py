"""scripts/measure.py, the protocol every scripts/*_rate.py measures by, without a device: the order of the event window against a fake torch that logs, the
rep loop's run order and its dropped warm-up, the spread rule, both JSON merges, the GPU requirement, bench_ab's order, environment and stop on a failed child
against a fake runner, and that each of the twelve scripts still starts (--help) with the module's prelude and no device."""
import contextlib
import importlib.util
import json
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = ("reference_rate", "instance_params_rate", "obstacle_mask_rate", "instance_bounds_rate", "sqp_rate", "obstacle_grid_rate", "sweep_rate", "multistart_rate",
           "rollout_merit_rate", "multistart_episode_rate", "multistart_sweep_rate", "multistart_geometry_rate")


@pytest.fixture(scope="module")
def measure():
    spec = importlib.util.spec_from_file_location("measure", os.path.join(ROOT, "scripts", "measure.py"))
    mod = importlib.util.module_from_spec(spec)
    path = list(sys.path)
    try:
        spec.loader.exec_module(mod)
        assert sys.path[:3] == [ROOT, os.path.join(ROOT, "dynamic-obstacle-avoidance-mpc_amd"), os.path.join(ROOT, "tests")]      # the prelude
    finally:
        sys.path[:] = path      # (the prelude is for a script's process, not for this one)
    return mod


class FakeTorch:
    """torch.cuda's events, streams and synchronize, each appending to .log; an event pair reads `elapsed_ms`"""

    def __init__(self, elapsed_ms=6.0):
        self.log, self.elapsed_ms, self.cuda = [], elapsed_ms, self
        self.device = lambda *a: a

    def synchronize(self):
        self.log.append("synchronize")

    def Event(self, enable_timing=False):
        assert enable_timing
        return types.SimpleNamespace(record=lambda stream: self.log.append(("record", stream.cuda_stream)), elapsed_time=lambda other: self.elapsed_ms)

    def Stream(self, device=None, handle=0x51):
        return types.SimpleNamespace(cuda_stream=handle, synchronize=lambda: self.log.append("stream.synchronize"))

    @contextlib.contextmanager
    def stream(self, st):
        self.log.append(("current", st.cuda_stream))
        yield
        self.log.append(("restored", st.cuda_stream))


def test_window_order_and_result(measure):
    t = FakeTorch(elapsed_ms=6.0)
    st = t.Stream()
    ms = measure.window(t, st, lambda: t.log.append("body"), 3, prepare=lambda: t.log.append("prepare"))
    assert t.log == ["prepare", "synchronize", ("record", 0x51), "body", "body", "body", ("record", 0x51), "synchronize"]
    assert ms == 2.0
    t.log.clear()
    assert measure.window(t, st, lambda: t.log.append("body"), 1) == 6.0
    assert t.log == ["synchronize", ("record", 0x51), "body", ("record", 0x51), "synchronize"]


def test_default_stream_is_refused(measure):
    t = FakeTorch()
    null = t.Stream(handle=0)
    with pytest.raises(ValueError):
        measure.window(t, null, lambda: t.log.append("body"), 3, prepare=lambda: t.log.append("prepare"))
    with pytest.raises(ValueError):
        measure.per_call(t, null, lambda: t.log.append("body"), 3)
    with pytest.raises(ValueError):
        with measure.own_stream(t, null):
            t.log.append("inside")
    assert t.log == []      # refused in front of everything


def test_own_stream_is_current_and_not_the_default(measure):
    t = FakeTorch()
    with measure.own_stream(t) as st:
        assert st.cuda_stream == 0x51
        t.log.append("inside")
    mine = t.Stream(handle=0x77)
    with measure.own_stream(t, mine) as st:
        assert st is mine
    assert t.log == [("current", 0x51), "inside", ("restored", 0x51), ("current", 0x77), ("restored", 0x77)]


def test_per_call_windows(measure):
    t = FakeTorch()
    t.Event = lambda enable_timing: types.SimpleNamespace(record=lambda s: t.log.append("record"), elapsed_time=lambda other: times[len(t.log) // 5 - 1])
    times = [0.004, 0.002, 0.009]
    r = measure.per_call(t, t.Stream(), lambda: t.log.append("body"), 3, prepare=lambda: t.log.append("prepare"))
    assert t.log == ["prepare", "record", "body", "record", "stream.synchronize"] * 3      # the stream is synchronised, never the device
    assert r == dict(median_us=pytest.approx(4.0), min_us=pytest.approx(2.0), max_us=pytest.approx(9.0))


def test_wall_synchronises_only_with_torch(measure):
    t = FakeTorch()
    seconds, r = measure.wall(lambda: t.log.append("call") or "result", t)
    assert t.log == ["synchronize", "call", "synchronize"] and r == "result" and seconds >= 0.0
    t.log.clear()
    assert measure.wall(lambda: t.log.append("call") or "result")[1] == "result" and t.log == ["call"]


def test_alternation(measure):
    order, seen = [], []
    count = iter(range(100))

    def form(name):
        return lambda: (order.append(name), next(count))[1]

    values = measure.alternate({f: form(f) for f in "abc"}, 3, on_run=lambda rep, f, v: seen.append((rep, f, v)))
    assert order == list("abc") * 4
    assert values == dict(a=[3, 6, 9], b=[4, 7, 10], c=[5, 8, 11])      # rep 0 returned 0, 1, 2: dropped
    assert seen == [(k // 3, "abc"[k % 3], k) for k in range(12)]      # the callback sees rep 0 too
    for reps in (0, -1):
        with pytest.raises(ValueError):
            measure.alternate(dict(a=form("a")), reps)
    assert order == list("abc") * 4      # refused in front of the first run


def test_summary(measure):
    assert measure.summary([2, 4, 9]) == (4.0, 1.75)
    assert measure.summary([9.0, 2.0, 4.0]) == (4.0, 1.75)
    assert measure.summary([3.5]) == (3.5, 0.0)
    assert all(type(v) is float for v in measure.summary([2, 4, 9]))
    assert measure.summaries(dict(x=[2, 4, 9], y=[5])) == (dict(x=4.0, y=5.0), dict(x=1.75, y=0.0))


ORDER = ["C2", "C3", "C5"]


def test_cell_merge_equal_header(measure, tmp_path):
    out = str(tmp_path / "rates.json")
    measure.merge_cells(out, dict(reps=5, steps_per_rep=20), [dict(cell="C5", v=1), dict(cell="C2", v=2)], ORDER)
    measure.merge_cells(out, dict(reps=5, steps_per_rep=20), [dict(cell="C3", v=3), dict(cell="C2", v=4)], ORDER)
    assert json.load(open(out)) == dict(reps=5, steps_per_rep=20, cells=[dict(cell="C2", v=4), dict(cell="C3", v=3), dict(cell="C5", v=1)])
    assert open(out).read().startswith('{\n "reps": 5,\n "steps_per_rep": 20,\n "cells": [\n  {')      # indent = 1, the header in front


def test_cell_merge_other_header_drops_the_old_cells(measure, tmp_path):
    out = str(tmp_path / "rates.json")
    measure.merge_cells(out, dict(reps=5, steps_per_rep=20), [dict(cell="C5", v=1), dict(cell="C2", v=2)], ORDER, extra=dict(rates=dict(K1=0.5)))
    measure.merge_cells(out, dict(reps=5, steps_per_rep=10), [dict(cell="C3", v=3)], ORDER, extra=dict(rates=None))
    assert json.load(open(out)) == dict(reps=5, steps_per_rep=10, cells=[dict(cell="C3", v=3)], rates=dict(K1=0.5))      # a None extra keeps the file's
    measure.merge_cells(out, dict(reps=5, steps_per_rep=10), [], ORDER, extra=dict(rates=dict(K1=0.75)))
    assert json.load(open(out)) == dict(reps=5, steps_per_rep=10, cells=[dict(cell="C3", v=3)], rates=dict(K1=0.75))


def test_merges_make_the_file_and_its_directory(measure, tmp_path):
    out = str(tmp_path / "not" / "there" / "rates.json")
    measure.merge_cells(out, dict(reps=1), [dict(cell="C3")], ORDER, extra=dict(rates=None))
    assert json.load(open(out)) == dict(reps=1, cells=[dict(cell="C3")], rates=None)
    parts = str(tmp_path / "nor" / "here" / "parts.json")
    assert measure.read_json(parts) == {}
    measure.write_json(parts, dict(a=1))
    assert json.load(open(parts)) == dict(a=1)


def test_part_merge_keeps_untouched_parts(measure, tmp_path):
    out = str(tmp_path / "parts.json")
    measure.write_json(out, dict(launch_times=dict(cells=[1, 2]), closed_loop=dict(runs=[3])))
    res = measure.read_json(out)
    res["closed_loop"] = dict(runs=[4])
    res["bench"] = dict(median=5)
    measure.write_json(out, res)
    assert json.load(open(out)) == dict(launch_times=dict(cells=[1, 2]), closed_loop=dict(runs=[4]), bench=dict(median=5))
    assert open(out).read().startswith('{\n "launch_times": {\n  "cells": [')


def test_gpu_requirement(measure, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)      # the real torch, on whichever machine: without a device there is no fallback
    with pytest.raises(SystemExit) as e:
        measure.require_gpu()
    assert e.value.code == "no GPU: this script measures on the device only"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    assert measure.require_gpu() is torch


class FakeRunner:
    """subprocess.run's stand-in: records each child's command, environment and limit, answers with a bench line of the next value"""

    def __init__(self, values, fail_at=None):
        self.values, self.fail_at, self.calls = list(values), fail_at, []

    def __call__(self, cmd, env, cwd, capture_output, text, timeout):
        k = len(self.calls)
        self.calls.append(dict(cmd=cmd, lib=env.get("MPC_GPU_LIB"), cwd=cwd, timeout=timeout))
        assert capture_output and text
        line = json.dumps(dict(value=self.values[k], unit="solves/s", ms_per_step=1.5, config=dict(mean_ipm_iters=11.0)))
        return types.SimpleNamespace(returncode=7 if k == self.fail_at else 0, stdout="a note\n" + line + "\n", stderr="")


def test_bench_ab_order_environment_and_figures(measure, tmp_path, monkeypatch, capsys):
    lib = tmp_path / "libparent.so"
    lib.write_bytes(b"")
    monkeypatch.setenv("MPC_GPU_LIB", "/left/over/from/the/caller.so")      # never reaches the `this` side
    run = FakeRunner([100.0, 90.0, 104.0, 95.0, 110.0, 99.0])
    r = measure.bench_ab(str(lib), 3, run=run)
    assert [c["lib"] for c in run.calls] == [str(lib), None] * 3
    assert all(c["timeout"] == 300 and c["cwd"] == measure.ROOT for c in run.calls)
    assert all(c["cmd"] == [sys.executable, os.path.join(measure.ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"] for c in run.calls)
    assert [(x["side"], x["round"], x["value"]) for x in r["runs"]] == [("parent", 0, 100.0), ("this", 0, 90.0), ("parent", 1, 104.0), ("this", 1, 95.0),
                                                                        ("parent", 2, 110.0), ("this", 2, 99.0)]
    assert r["runs"][0] == dict(side="parent", round=0, value=100.0, unit="solves/s", ms_per_step=1.5, mean_ipm_iters=11.0)
    assert r["order"] == "parent, this" and r["command"] == "bench.py --gpus 1 --steps 20 --warmup 5"
    assert r["median"] == dict(parent=104.0, this=95.0)
    assert r["this_over_parent"] == 95.0 / 104.0 and r["parent_spread"] == (110.0 - 100.0) / 104.0
    assert sorted(r) == ["command", "median", "order", "parent_spread", "runs", "this_over_parent"]
    assert len(capsys.readouterr().out.splitlines()) == 6      # one progress line per child


def test_bench_ab_this_first(measure, tmp_path):
    lib = tmp_path / "libparent.so"
    lib.write_bytes(b"")
    run = FakeRunner([90.0, 100.0, 95.0, 104.0])
    r = measure.bench_ab(str(lib), 2, this_first=True, run=run)
    assert [c["lib"] for c in run.calls] == [None, str(lib)] * 2
    assert [x["side"] for x in r["runs"]] == ["this", "parent"] * 2 and r["order"] == "this, parent"
    assert r["median"] == dict(parent=102.0, this=92.5)


def test_bench_ab_starts_nothing_behind_a_failed_child(measure, tmp_path):
    lib = tmp_path / "libparent.so"
    lib.write_bytes(b"")
    run = FakeRunner([100.0] * 6, fail_at=1)
    with pytest.raises(SystemExit) as e:
        measure.bench_ab(str(lib), 3, run=run)
    assert len(run.calls) == 2 and "(this, round 0) ended with 7" in str(e.value.code)
    none = FakeRunner([])
    with pytest.raises(SystemExit):
        measure.bench_ab(str(tmp_path / "missing.so"), 3, run=none)
    assert none.calls == []


@pytest.mark.parametrize("name", SCRIPTS)
def test_script_starts_without_a_device(name):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", name + ".py"), "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.startswith("usage: " + name + ".py")
