"""Seed sweeps without a device: the slot-order model (refill_schedule), the agreement of header, symbol table and binding on mpc_episode_refill_dev,
and run_seed_sweep's refusals, which happen before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def ep():
    import mpc_gpu.episodes as ep       # (pure Python: no library is loaded by the import)
    return ep


# ---------------------------------------------------------------------------------------------------------------- 1. the schedule model
def test_equal_lengths_refill_in_lockstep(ep):
    r = ep.refill_schedule([7] * 10, 4)
    assert r["slot"].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]
    assert r["start"].tolist() == [0, 0, 0, 0, 7, 7, 7, 7, 14, 14]
    assert r["steps"] == 21


def test_one_long_episode_and_the_other_slots_cycle(ep):
    r = ep.refill_schedule([100, 3, 3, 3, 3, 3, 3], 3)
    assert r["slot"].tolist() == [0, 1, 2, 1, 2, 1, 2]
    assert r["start"].tolist() == [0, 0, 0, 3, 3, 6, 6]
    assert r["steps"] == 100
    r = ep.refill_schedule([2, 2, 2, 2, 50], 2)          # the long one last: it is the tail
    assert r["slot"].tolist() == [0, 1, 0, 1, 0] and r["start"].tolist() == [0, 0, 2, 2, 4] and r["steps"] == 54


def test_more_slots_than_seeds(ep):
    r = ep.refill_schedule([5, 9, 2], 8)
    assert r["slot"].tolist() == [0, 1, 2] and r["start"].tolist() == [0, 0, 0] and r["steps"] == 9


def test_slots_that_finish_in_the_same_step_are_served_in_slot_order(ep):
    # slots 0, 1, 2 run 4, 2 + 2, 4 steps: in front of step 4 all three are free, and seeds 4, 5, 6 go to slots 0, 1, 2 in that order
    r = ep.refill_schedule([4, 2, 4, 2, 1, 1, 1], 3)
    assert r["slot"].tolist() == [0, 1, 2, 1, 0, 1, 2]
    assert r["start"].tolist() == [0, 0, 0, 2, 4, 4, 4]
    assert r["steps"] == 5
    # a later slot that frees EARLIER is served first: slot order breaks ties of one step only
    r = ep.refill_schedule([5, 1, 9, 9], 2)
    assert r["slot"].tolist() == [0, 1, 1, 0] and r["start"].tolist() == [0, 0, 1, 5] and r["steps"] == 14


def test_the_schedule_never_outruns_the_loop_bound(ep):
    """ceil(count / slots) * max_iter bounds every schedule of episodes of at most max_iter steps (the bound run_seed_sweep's loop carries)"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        count, slots, cap = int(rng.integers(1, 40)), int(rng.integers(1, 9)), int(rng.integers(1, 30))
        lengths = rng.integers(1, cap + 1, count)
        if rng.random() < 0.5:
            lengths[rng.integers(0, count, max(1, count // 2))] = cap
        r = ep.refill_schedule(lengths, slots)
        S = min(slots, count)
        assert r["steps"] <= -(-count // S) * cap
        assert r["steps"] >= max(int(lengths.max()), -(-int(lengths.sum()) // S))
        assert sorted(r["slot"][:S].tolist()) == list(range(S)) and (r["start"][:S] == 0).all()


def test_schedule_model_refuses_nonsense(ep):
    for bad in ([3, 0, 2], [1.5, 2], [[1, 2]]):
        with pytest.raises(ValueError):
            ep.refill_schedule(bad, 2)
    with pytest.raises(ValueError):
        ep.refill_schedule([1, 2], 0)


# ---------------------------------------------------------------------------------------------------------------- 2. header, symbol table, binding
def header_text():
    return open(os.path.join(ROOT, "include", "mpc_gpu.h")).read()


def header_prototype(name):
    src = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, name
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    out = []
    for p in params:
        pname = re.search(r"(\w+)$", p).group(1)
        ptype = p[:-len(pname)].strip()
        out.append((ptype, pname))
    return out


def test_header_symbols_and_binding_agree_on_the_refill_entry_point(monkeypatch):
    from mpc_gpu import _lib
    from mpc_gpu.solver import BatchedMpc
    proto = header_prototype("mpc_episode_refill_dev")
    ctype = lambda t: _lib._vp if t.endswith("*") else {"int": C.c_int, "unsigned": C.c_uint}[t]
    res, args = _lib.SYMBOLS["mpc_episode_refill_dev"]
    assert res is C.c_int and args == [ctype(t) for t, _ in proto]
    assert [n for _, n in proto][:7] == ["h", "slots", "scenario", "seed_first", "seed_count", "max_steps", "flags"] and proto[-1] == ("void *", "stream")
    # the binding hands every argument to the position the header gives it: distinct integers stand in for the device pointers
    seen = {}

    class Fake:
        def mpc_episode_refill_dev(self, *a):
            seen["args"] = a
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    m = object.__new__(BatchedMpc)
    m._h = C.c_void_p(4096)
    ptr_names = [n for t, n in proto if t.endswith("*") and n not in ("h", "box")]
    vals = {n: 1000 + 8 * i for i, n in enumerate(ptr_names)}
    py = lambda n: n[2:] if n.startswith("d_") else n
    try:
        m.episode_refill_dev(slots=6, scenario="EDGE", seed_first=37, seed_count=10, max_steps=400, per_seed=True, flags=5,
                             **{py(n): v for n, v in vals.items()})
    finally:
        m._h = C.c_void_p()          # (not a handle of its own: nothing for close() to destroy)
    got = seen["args"]
    assert len(got) == len(proto)
    for (t, n), a in zip(proto, got):
        if n == "h":
            assert a.value == 4096
        elif n == "box":
            assert isinstance(a, C.c_void_p) and a.value
        elif t.endswith("*"):
            assert a.value == vals[n], n
        else:
            assert a == dict(slots=6, scenario=2, seed_first=37, seed_count=10, max_steps=400, flags=5, per_seed=1)[n], n


def test_refill_flags_are_distinct_bits_and_mirror_the_header():
    from mpc_gpu import _lib
    hdr = header_text()
    vals = {n: int(re.search(r"#define\s+MPC_REFILL_" + n + r"\s+(\d+)", hdr).group(1)) for n in ("ALIAS_BUG", "INTERP_GUESS", "DRAW_NOISE")}
    assert vals == dict(ALIAS_BUG=_lib.REFILL_ALIAS_BUG, INTERP_GUESS=_lib.REFILL_INTERP_GUESS, DRAW_NOISE=_lib.REFILL_DRAW_NOISE)
    assert all(v > 0 and v & (v - 1) == 0 for v in vals.values()) and len(set(vals.values())) == 3
    assert int(re.search(r"#define\s+MPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 7 == _lib.ABI_VERSION      # additive: no struct, no signature changed


# ---------------------------------------------------------------------------------------------------------------- 3. refusals before any device call
@pytest.fixture
def no_device(monkeypatch):
    """any attempt to load the library or to create a handle fails the test"""
    from mpc_gpu import _lib
    from mpc_gpu.solver import BatchedMpc

    def touched(*a, **k):
        raise AssertionError("a refusal must not touch the device")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(BatchedMpc, "__init__", touched)


def test_run_seed_sweep_refuses_before_any_device_call(ep, no_device):
    start, goal = [-7.0, -7.0, np.pi / 4, 0, 0], [7.0, 7.0]
    with pytest.raises(ValueError, match="step 1"):
        ep.run_seed_sweep(start, goal, "RANDOM", range(0, 20, 2), 4)
    with pytest.raises(ValueError, match="per-seed start"):
        ep.run_seed_sweep(np.zeros((7, 5)), goal, "RANDOM", (0, 10), 4)
    with pytest.raises(ValueError, match="per-seed goal"):
        ep.run_seed_sweep(start, np.zeros((3, 2)), "RANDOM", range(10), 4)
    with pytest.raises(ValueError, match="slots"):
        ep.run_seed_sweep(start, goal, "RANDOM", (0, 10), 0)
    with pytest.raises(ValueError, match="scenario name"):
        ep.run_seed_sweep(start, goal, np.zeros((10, 5, 4)), (0, 10), 4)
    with pytest.raises(ValueError, match="unknown scenario"):
        ep.run_seed_sweep(start, goal, "CORNER", (0, 10), 4)
    with pytest.raises(ValueError):
        ep.run_seed_sweep(start, goal, "RANDOM", (0, 0), 4)
    with pytest.raises(ValueError):
        ep.run_seed_sweep(start, goal, "RANDOM", 10, 4)
    with pytest.raises(TypeError):           # not offered: there is no such argument
        ep.run_seed_sweep(start, goal, "RANDOM", (0, 10), 4, record=True, r_safe=np.ones(10))


def test_sweep_arguments_are_normalised(ep):
    first, count, start, goal, per_seed = ep._sweep_arguments([0, 1, 2, 3, 4], [5, 6], "EDGE", range(37, 47), 3, 400, 25)
    assert (first, count, per_seed) == (37, 10, False) and start.shape == (1, 5) and goal.shape == (1, 2)
    rows = np.arange(50.0).reshape(10, 5)
    first, count, start, goal, per_seed = ep._sweep_arguments(rows, [5, 6], "EDGE", (37, 10), 3, 400, 25)
    assert per_seed and start.shape == (10, 5) and goal.shape == (10, 2) and (goal == [5, 6]).all() and (start == rows).all()
    assert start.flags["C_CONTIGUOUS"] and goal.flags["C_CONTIGUOUS"]
